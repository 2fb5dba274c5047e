// Noise-driven per-pixel sample counts (ptx_render_adaptive, ptx_adaptive_select, ptx_accum_mean; the specification is in include/ptx.h and
// DESIGN.md §5.6). The reference has no adaptive sampling: every value here is defined by that text, IEEE binary32, one rounding per
// operation in the written parenthesisation; there is no libm call on this path.
//   k_ad_noisy     per pixel: the two half-buffers' means -> one byte, 1 = the halves disagree by more than the threshold (NaN: noisy)
//   k_ad_decide    one workgroup of four waves per 32 x 32 tile, one wave-iteration per 8 x 8 block (lane = ry * 8 + rx): the 3 x 3 dilation of
//                  the noisy bytes clipped to the rectangle, the `done` latch, one __ballot per block -> the block's 64-bit active mask and
//                  its offset inside the tile, and the tile's count
//   k_ad_scan      exclusive scan of the tile counts (one workgroup) -> tile offsets and the number of active pixels
//   k_ad_scatter   the same geometry as k_ad_decide: a lane whose bit is set writes its pixel at tile offset + block offset + mbcnt rank
// The list is a function of the masks alone (no atomics): tiles row-major, the 8 x 8 blocks of a tile row-major, rows inside a block.
// Under interleaved tile sharding with a mask exchange (ptx_ctx_set_mask_exchange) a rank runs, beside the kernels above and without touching them:
//   k_ad_noisy_shard   the noisy rule for the rank's own pixels, 0 for the others (their sums are zeros here: 0 / 0 would read as noisy)
//   k_ad_decide_shard  k_ad_decide on the MERGED mask (nonzero = noisy): `done` is latched for every pixel of the rectangle, and a block takes two
//                      ballots: all active pixels, of which only the count is kept, and the rank's own, which feed k_ad_scatter as they are
//   k_ad_scan_shard    k_ad_scan of the own counts, and the sum of the all-pixels counts: two totals from one launch
//   k_ad_mean      (a + b) / (a.w + b.w), or a / a.w: the frame of unequal per-pixel counts as MEANS
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ptx {

constexpr int kAdScanThreads = 1024;

__global__ void __launch_bounds__(256) k_ad_noisy(const float4* __restrict__ a, const float4* __restrict__ b, uint32_t n_pixels, float threshold,
                                                  uint8_t* __restrict__ noisy) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 A = a[p], B = b[p];
	const float ar = A.x / A.w, ag = A.y / A.w, ab = A.z / A.w;
	const float br = B.x / B.w, bg = B.y / B.w, bb = B.z / B.w;
	const float d = (fabsf(ar - br) + fabsf(ag - bg)) + fabsf(ab - bb);
	const float m = ((ar + br) + (ag + bg)) + (ab + bb);
	const float e2 = ((d * d) * 0.25f) / fmaxf(m * 0.5f, 0.01f);
	noisy[p] = !(e2 <= threshold * threshold) ? 1 : 0;   // a NaN is noisy: a pixel is never stopped on garbage
}

// the pixel of lane `lane` of block `blk` (0 .. 15, row-major) of the tile; false: outside the rectangle
__device__ __forceinline__ bool ad_pixel(uint32_t w, uint32_t h, uint32_t blk, uint32_t lane, uint32_t& x, uint32_t& y) {
	x = blockIdx.x * kAdTile + (blk & 3u) * 8u + (lane & 7u);
	y = blockIdx.y * kAdTile + (blk >> 2) * 8u + (lane >> 3);
	return x < w && y < h;
}

__global__ void __launch_bounds__(256) k_ad_decide(const uint8_t* __restrict__ noisy, uint32_t w, uint32_t h, uint8_t* __restrict__ done,
                                                   unsigned long long* __restrict__ block_mask, uint32_t* __restrict__ block_off, uint32_t* __restrict__ tile_count) {
	__shared__ uint32_t s_cnt[kAdBlocksPerTile];
	const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t blk = wave * 4u + k;
		uint32_t x, y;
		bool active = false;
		if (ad_pixel(w, h, blk, lane, x, y)) {
			const uint32_t xa = x > 0 ? x - 1 : 0, xb = x + 1 < w ? x + 1 : w - 1, ya = y > 0 ? y - 1 : 0, yb = y + 1 < h ? y + 1 : h - 1;   // clipped to the rectangle
			uint32_t any = 0;
			for (uint32_t qy = ya; qy <= yb; qy++)
				for (uint32_t qx = xa; qx <= xb; qx++) any |= noisy[qy * w + qx];
			const uint32_t p = y * w + x;
			active = !done[p] && any;
			done[p] = active ? 0 : 1;   // the latch: done |= !active
		}
		const unsigned long long mask = __ballot(active);
		if (lane == 0) {
			block_mask[tile * kAdBlocksPerTile + blk] = mask;
			s_cnt[blk] = (uint32_t)__popcll(mask);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t sum = 0;
		for (uint32_t blk = 0; blk < kAdBlocksPerTile; blk++) {
			block_off[tile * kAdBlocksPerTile + blk] = sum;
			sum += s_cnt[blk];
		}
		tile_count[tile] = sum;
	}
}

// one workgroup: thread t sums the counts of its run of `per` tiles, the 1024 run sums are scanned in LDS, and t writes its run's offsets
__global__ void __launch_bounds__(kAdScanThreads) k_ad_scan(const uint32_t* __restrict__ tile_count, uint32_t n_tiles, uint32_t* __restrict__ tile_off, uint32_t* __restrict__ n_active) {
	__shared__ uint32_t s_sum[kAdScanThreads];
	const uint32_t t = threadIdx.x, per = (n_tiles + kAdScanThreads - 1) / kAdScanThreads;
	const uint32_t first = t * per < n_tiles ? t * per : n_tiles, last = first + per < n_tiles ? first + per : n_tiles;
	uint32_t sum = 0;
	for (uint32_t i = first; i < last; i++) sum += tile_count[i];
	s_sum[t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kAdScanThreads; step <<= 1) {   // inclusive Hillis-Steele scan
		const uint32_t add = t >= step ? s_sum[t - step] : 0;
		__syncthreads();
		s_sum[t] += add;
		__syncthreads();
	}
	uint32_t off = s_sum[t] - sum;
	for (uint32_t i = first; i < last; i++) {
		tile_off[i] = off;
		off += tile_count[i];
	}
	if (t == kAdScanThreads - 1) *n_active = s_sum[t];
}

// the rank that owns pixel (lx, ly) of the rectangle: the row-major index of its shard tile in the FULL image, modulo the number of ranks
struct AdShard {
	uint32_t x0, y0, ts, tiles_x, index, count;
	__device__ __forceinline__ bool owns(uint32_t lx, uint32_t ly) const { return (((y0 + ly) / ts) * tiles_x + (x0 + lx) / ts) % count == index; }
};

__global__ void __launch_bounds__(256) k_ad_noisy_shard(const float4* __restrict__ a, const float4* __restrict__ b, uint32_t w, uint32_t n_pixels, float threshold, AdShard S,
                                                        uint8_t* __restrict__ mask) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n_pixels) return;
	uint8_t noisy = 0;
	if (S.owns(p % w, p / w)) {
		const float4 A = a[p], B = b[p];
		const float ar = A.x / A.w, ag = A.y / A.w, ab = A.z / A.w;
		const float br = B.x / B.w, bg = B.y / B.w, bb = B.z / B.w;
		const float d = (fabsf(ar - br) + fabsf(ag - bg)) + fabsf(ab - bb);
		const float m = ((ar + br) + (ag + bg)) + (ab + bb);
		const float e2 = ((d * d) * 0.25f) / fmaxf(m * 0.5f, 0.01f);
		noisy = !(e2 <= threshold * threshold) ? 1 : 0;
	}
	mask[p] = noisy;
}

__global__ void __launch_bounds__(256) k_ad_decide_shard(const uint8_t* __restrict__ merged, uint32_t w, uint32_t h, AdShard S, uint8_t* __restrict__ done,
                                                         unsigned long long* __restrict__ block_mask, uint32_t* __restrict__ block_off, uint32_t* __restrict__ tile_count,
                                                         uint32_t* __restrict__ tile_count_all) {
	__shared__ uint32_t s_cnt[kAdBlocksPerTile], s_all[kAdBlocksPerTile];
	const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t blk = wave * 4u + k;
		uint32_t x, y;
		bool active = false, own = false;
		if (ad_pixel(w, h, blk, lane, x, y)) {
			const uint32_t xa = x > 0 ? x - 1 : 0, xb = x + 1 < w ? x + 1 : w - 1, ya = y > 0 ? y - 1 : 0, yb = y + 1 < h ? y + 1 : h - 1;   // clipped to the rectangle
			uint32_t any = 0;
			for (uint32_t qy = ya; qy <= yb; qy++)
				for (uint32_t qx = xa; qx <= xb; qx++) any |= merged[qy * w + qx];   // any nonzero byte is noisy: MAX, OR and SUM merges all serve
			const uint32_t p = y * w + x;
			active = !done[p] && any;
			done[p] = active ? 0 : 1;   // the latch, for every pixel: all ranks hold the same `done`
			own = active && S.owns(x, y);   // shard tiles need not be multiples of 8: per lane
		}
		const unsigned long long all = __ballot(active), mask = __ballot(own);
		if (lane == 0) {
			block_mask[tile * kAdBlocksPerTile + blk] = mask;
			s_cnt[blk] = (uint32_t)__popcll(mask);
			s_all[blk] = (uint32_t)__popcll(all);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t sum = 0, sum_all = 0;
		for (uint32_t blk = 0; blk < kAdBlocksPerTile; blk++) {
			block_off[tile * kAdBlocksPerTile + blk] = sum;
			sum += s_cnt[blk];
			sum_all += s_all[blk];
		}
		tile_count[tile] = sum;
		tile_count_all[tile] = sum_all;
	}
}

// k_ad_scan of the own counts -> tile offsets and n_active[0]; the all-pixels counts are only summed -> n_active[1]
__global__ void __launch_bounds__(kAdScanThreads) k_ad_scan_shard(const uint32_t* __restrict__ tile_count, const uint32_t* __restrict__ tile_count_all, uint32_t n_tiles,
                                                                  uint32_t* __restrict__ tile_off, uint32_t* __restrict__ n_active) {
	__shared__ uint32_t s_sum[kAdScanThreads];
	__shared__ uint32_t s_all;
	const uint32_t t = threadIdx.x, per = (n_tiles + kAdScanThreads - 1) / kAdScanThreads;
	const uint32_t first = t * per < n_tiles ? t * per : n_tiles, last = first + per < n_tiles ? first + per : n_tiles;
	uint32_t sum = 0, sum_all = 0;
	for (uint32_t i = first; i < last; i++) {
		sum += tile_count[i];
		sum_all += tile_count_all[i];
	}
	s_sum[t] = sum;
	if (t == 0) s_all = 0;
	__syncthreads();
	if (sum_all) atomicAdd(&s_all, sum_all);   // an integer sum: the order does not matter
	for (uint32_t step = 1; step < kAdScanThreads; step <<= 1) {   // inclusive Hillis-Steele scan
		const uint32_t add = t >= step ? s_sum[t - step] : 0;
		__syncthreads();
		s_sum[t] += add;
		__syncthreads();
	}
	uint32_t off = s_sum[t] - sum;
	for (uint32_t i = first; i < last; i++) {
		tile_off[i] = off;
		off += tile_count[i];
	}
	if (t == kAdScanThreads - 1) {
		n_active[0] = s_sum[t];
		n_active[1] = s_all;
	}
}

__global__ void __launch_bounds__(256) k_ad_scatter(const unsigned long long* __restrict__ block_mask, const uint32_t* __restrict__ block_off, const uint32_t* __restrict__ tile_off,
                                                    uint32_t w, uint32_t h, uint32_t* __restrict__ pixels) {
	const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t base = tile_off[tile];
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t blk = wave * 4u + k;
		const unsigned long long mask = block_mask[tile * kAdBlocksPerTile + blk];
		uint32_t x, y;
		ad_pixel(w, h, blk, lane, x, y);   // a set bit is a pixel inside the rectangle
		// the lane's rank among the set bits below it
		const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
		if ((mask >> lane) & 1ull) pixels[base + block_off[tile * kAdBlocksPerTile + blk] + rank] = y * w + x;
	}
}

template <bool TWO>
__global__ void __launch_bounds__(256) k_ad_mean(const float4* a, const float4* b, size_t n_pixels, float4* out) {   // out may be a or b: a thread reads its pixel before it writes it
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (p >= n_pixels) return;
	const float4 A = a[p];
	if constexpr (TWO) {
		const float4 B = b[p];
		const float n = A.w + B.w;
		out[p] = make_float4((A.x + B.x) / n, (A.y + B.y) / n, (A.z + B.z) / n, (A.w + B.w) / n);
	} else {
		out[p] = make_float4(A.x / A.w, A.y / A.w, A.z / A.w, A.w / A.w);
	}
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_adaptive_select(const float4* a, const float4* b, uint32_t w, uint32_t h, float threshold, const AdaptiveBuffers& B, uint8_t* done, uint32_t* pixels,
                                  hipStream_t stream) {
	const uint32_t n = w * h;
	const dim3 tiles((w + kAdTile - 1) / kAdTile, (h + kAdTile - 1) / kAdTile);
	hipLaunchKernelGGL(k_ad_noisy, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, b, n, threshold, B.noisy);
	hipLaunchKernelGGL(k_ad_decide, tiles, dim3(256), 0, stream, B.noisy, w, h, done, B.block_mask, B.block_off, B.tile_count);
	hipLaunchKernelGGL(k_ad_scan, dim3(1), dim3(kAdScanThreads), 0, stream, B.tile_count, tiles.x * tiles.y, B.tile_off, B.n_active);
	if (pixels) hipLaunchKernelGGL(k_ad_scatter, tiles, dim3(256), 0, stream, B.block_mask, B.block_off, B.tile_off, w, h, pixels);
	return hipGetLastError();
}

hipError_t launch_adaptive_noisy_shard(const float4* a, const float4* b, uint32_t w, uint32_t h, float threshold, const AdaptiveShard& shard, uint8_t* mask, hipStream_t stream) {
	const uint32_t n = w * h;
	const AdShard S{shard.x0, shard.y0, shard.ts, shard.tiles_x, shard.index, shard.count};
	hipLaunchKernelGGL(k_ad_noisy_shard, dim3((n + 255u) / 256u), dim3(256), 0, stream, a, b, w, n, threshold, S, mask);
	return hipGetLastError();
}

hipError_t launch_adaptive_decide_shard(const uint8_t* merged, uint32_t w, uint32_t h, const AdaptiveShard& shard, const AdaptiveBuffers& B, uint32_t* tile_count_all, uint8_t* done,
                                        uint32_t* pixels, hipStream_t stream) {
	const dim3 tiles((w + kAdTile - 1) / kAdTile, (h + kAdTile - 1) / kAdTile);
	const AdShard S{shard.x0, shard.y0, shard.ts, shard.tiles_x, shard.index, shard.count};
	hipLaunchKernelGGL(k_ad_decide_shard, tiles, dim3(256), 0, stream, merged, w, h, S, done, B.block_mask, B.block_off, B.tile_count, tile_count_all);
	hipLaunchKernelGGL(k_ad_scan_shard, dim3(1), dim3(kAdScanThreads), 0, stream, B.tile_count, tile_count_all, tiles.x * tiles.y, B.tile_off, B.n_active);
	hipLaunchKernelGGL(k_ad_scatter, tiles, dim3(256), 0, stream, B.block_mask, B.block_off, B.tile_off, w, h, pixels);
	return hipGetLastError();
}

hipError_t launch_accum_mean(const float4* a, const float4* b, size_t n_pixels, float4* out, hipStream_t stream) {
	const dim3 grid((unsigned)((n_pixels + 255) / 256));
	if (b) hipLaunchKernelGGL(k_ad_mean<true>, grid, dim3(256), 0, stream, a, b, n_pixels, out);
	else hipLaunchKernelGGL(k_ad_mean<false>, grid, dim3(256), 0, stream, a, b, n_pixels, out);
	return hipGetLastError();
}

}  // namespace ptx
