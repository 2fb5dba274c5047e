// Temporal accumulation in front of the a-trous filter (ptx_denoise_temporal and ptx_denoise_temporal_counts; the specifications are in
// include/ptx.h and DESIGN.md §5.9 and §5.10).
//   k_tp_accumulate   per pixel: step 1 of the filter (what k_dn_prepare computes), the reprojection of last frame's history through the
//                     pixel's mean motion (four bilinear taps, each tested against the expected depth and the current normal), the blend,
//                     the variance the filter starts from, and the history of the next frame. It replaces k_dn_prepare; everything after
//                     it is the filter's own (denoise.hip).
// The history holds the accumulated UNFILTERED colour: the filter's blur never feeds back, so it does not compound over the frames.
// Numerics as in denoise.hip: IEEE binary32, one rounding per operation in the written parenthesisation, no contraction.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ptx {

constexpr int kTpBlockX = 64, kTpBlockY = 4;   // one wave per 64-pixel row segment, as k_dn_prefilter

__device__ __forceinline__ float tp_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the normal test of a tap: the dot product with the tap's stored mean normal, or (UNIT) with its direction
template <bool UNIT>
__device__ __forceinline__ float tp_normal_dot(const float4& up, const float4& q) {
	if constexpr (UNIT) {
		const float lq = sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);   // a zero normal: 0 / 0 = NaN, the test fails
		return (up.x * (q.x / lq) + up.y * (q.y / lq)) + up.z * (q.z / lq);
	} else {
		return (up.x * q.x + up.y * q.y) + up.z * q.z;
	}
}

// H.prev_* == nullptr: the first frame, no pixel has a history. col_var == nullptr: the caller only advances the history.
// counter: reprojected pixels in the low 32 bits, pixels that started over in the high 32 (W * H <= 2^28), one atomic per wave, into the
// slot of the wave's workgroup (kernels.hpp: kTpCounterSlots).
// COUNTS (ptx_denoise_temporal_counts): the halves carry per-pixel sample counts in .w, T.n is float(guide_spp), the history length counts
// SAMPLES. UNIT: the normal test compares unit normals. SEARCH: a pixel whose four taps all failed looks at the 3 x 3 texels around the
// rounded previous position. <false, false, false> is ptx_denoise_temporal's kernel: its arguments and its arithmetic are what they were.
template <bool COUNTS, bool SEARCH, bool UNIT>
__global__ void __launch_bounds__(kTpBlockX* kTpBlockY) k_tp_accumulate(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ albedo_cov,
                                                                       const float4* __restrict__ normal_depth, const float4* __restrict__ motion, TemporalHistory prev,
                                                                       TemporalHistory next, TemporalParams T, float4* __restrict__ col_var, float4* __restrict__ guide,
                                                                       float4* __restrict__ remod, unsigned long long* __restrict__ counter) {
	const int x = blockIdx.x * kTpBlockX + threadIdx.x, y = blockIdx.y * kTpBlockY + threadIdx.y;
	const bool inside = x < T.W && y < T.H;
	bool took = false;
	if (inside) {
		const size_t p = (size_t)y * T.W + x;
		const float4 A = a[p], B = b[p], G = albedo_cov[p], N = normal_depth[p], M = motion[p];
		// 1. the current frame: k_dn_prepare's arithmetic (COUNTS: k_dn_prepare_counts'; ng = the guides' samples)
		const float na = COUNTS ? A.w : T.na, nb = COUNTS ? B.w : T.nb, n = COUNTS ? na + nb : T.n, ng = T.n;
		const float cov = G.w, miss = ng - cov;
		const float ax = fmaxf((G.x + miss) / ng, 0.001f), ay = fmaxf((G.y + miss) / ng, 0.001f), az = fmaxf((G.z + miss) / ng, 0.001f);
		const float d = (tp_lum((A.x / na) / ax, (A.y / na) / ay, (A.z / na) / az) - tp_lum((B.x / nb) / ax, (B.y / nb) / ay, (B.z / nb) / az)) * 0.5f;
		const float cr = ((A.x + B.x) / n) / ax, cg = ((A.y + B.y) / n) / ay, cb = ((A.z + B.z) / n) / az, v0 = d * d;
		const float4 g = cov > 0.0f ? make_float4(N.x / cov, N.y / cov, N.z / cov, N.w / cov) : make_float4(0.f, 0.f, 0.f, 0.f);
		const float L = tp_lum(cr, cg, cb), LL = L * L;

		// 2. reprojection
		bool have = prev.color != nullptr && M.w > 0.0f;
		const float mvx = M.x / M.w, mvy = M.y / M.w, zexp = M.z / M.w;
		const float gx = (((float)x + 0.5f) + mvx) - 0.5f, gy = (((float)y + 0.5f) + mvy) - 0.5f;
		have = have && fabsf(gx) < 32768.0f && fabsf(gy) < 32768.0f;   // NaN fails
		const float flx = floorf(gx), fly = floorf(gy);
		const float wx = gx - flx, wy = gy - fly;
		const int ix = have ? (int)flx : 0, iy = have ? (int)fly : 0;
		// what the normal test multiplies the tap's normal with: the mean normal, or (UNIT) its direction
		float4 up = g;
		if constexpr (UNIT) {
			const float lp = sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z);
			up = make_float4(g.x / lp, g.y / lp, g.z / lp, g.w);
		}
		float sw = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, h1 = 0.0f, h2 = 0.0f;
		if (prev.color != nullptr) {   // uniform over the launch
			// the four taps' fetches, at coordinates clamped to the image, are issued together; what a tap outside the image fetched is never used
			float4 qc[4], qg[4];
			float2 qm[4];
#pragma unroll
			for (int t = 0; t < 4; t++) {
				const int qx = ix + (t & 1), qy = iy + (t >> 1);
				const size_t q = (size_t)(qy < 0 ? 0 : (qy >= T.H ? T.H - 1 : qy)) * T.W + (qx < 0 ? 0 : (qx >= T.W ? T.W - 1 : qx));
				qc[t] = prev.color[q];
				qm[t] = prev.moments[q];
				qg[t] = prev.geometry[q];
			}
#pragma unroll
			for (int t = 0; t < 4; t++) {   // dy outer, dx inner
				const int dx = t & 1, dy = t >> 1, qx = ix + dx, qy = iy + dy;
				const float bq = (dx ? wx : 1.0f - wx) * (dy ? wy : 1.0f - wy);
				const float4 c = qc[t], q = qg[t];
				const bool take = have && qx >= 0 && qx < T.W && qy >= 0 && qy < T.H && bq > 0.0f && c.w > 0.0f && q.w > 0.0f &&
				                  fabsf(zexp - q.w) <= T.tau_z * fmaxf(zexp, q.w) && tp_normal_dot<UNIT>(up, q) >= T.tau_n;
				// a tap that is not taken adds nothing, not even 0 * NaN
				sw = take ? sw + bq : sw;
				hr = take ? hr + bq * c.x : hr;
				hg = take ? hg + bq * c.y : hg;
				hb = take ? hb + bq * c.z : hb;
				hn = take ? hn + bq * c.w : hn;
				h1 = take ? h1 + bq * qm[t].x : h1;
				h2 = take ? h2 + bq * qm[t].y : h2;
			}
			if constexpr (SEARCH) {
				// only the lanes whose motion was usable and whose four taps all failed: the nine texels around the rounded previous position,
				// each with weight 1. One row's nine fetches are issued together, clamped as above.
				if (have && sw == 0.0f) {
					const int rx = (int)floorf(gx + 0.5f), ry = (int)floorf(gy + 0.5f);   // |gx|, |gy| < 32768
#pragma nounroll
					for (int dy = -1; dy <= 1; dy++) {
						const int qy = ry + dy;
						const size_t row = (size_t)(qy < 0 ? 0 : (qy >= T.H ? T.H - 1 : qy)) * T.W;
						float4 sc[3], sg[3];
						float2 sm[3];
#pragma unroll
						for (int dx = -1; dx <= 1; dx++) {
							const int qx = rx + dx;
							const size_t q = row + (qx < 0 ? 0 : (qx >= T.W ? T.W - 1 : qx));
							sc[dx + 1] = prev.color[q];
							sm[dx + 1] = prev.moments[q];
							sg[dx + 1] = prev.geometry[q];
						}
#pragma unroll
						for (int dx = -1; dx <= 1; dx++) {
							const int qx = rx + dx;
							const float4 c = sc[dx + 1], q = sg[dx + 1];
							const bool take = qx >= 0 && qx < T.W && qy >= 0 && qy < T.H && c.w > 0.0f && q.w > 0.0f &&
							                  fabsf(zexp - q.w) <= T.tau_z * fmaxf(zexp, q.w) && tp_normal_dot<UNIT>(up, q) >= T.tau_n;
							sw = take ? sw + 1.0f : sw;
							hr = take ? hr + c.x : hr;
							hg = take ? hg + c.y : hg;
							hb = take ? hb + c.z : hb;
							hn = take ? hn + c.w : hn;
							h1 = take ? h1 + sm[dx + 1].x : h1;
							h2 = take ? h2 + sm[dx + 1].y : h2;
						}
					}
				}
			}
		}
		have = have && sw > 0.0f;
		hr = hr / sw; hg = hg / sw; hb = hb / sw; hn = hn / sw; h1 = h1 / sw; h2 = h2 / sw;

		// 3. blend; a pixel whose blend is not finite starts over. The frame weighs 1 of N' frames, or (COUNTS) n of N' samples
		const float Nh = COUNTS ? fminf(hn + n, fmaxf(T.max_history, n)) : fminf(hn + 1.0f, T.max_history);
		const float al = (COUNTS ? n : 1.0f) / Nh;
		const float br = hr + (cr - hr) * al, bg = hg + (cg - hg) * al, bb = hb + (cb - hb) * al;
		const float b1 = h1 + (L - h1) * al, b2 = h2 + (LL - h2) * al;
		took = have && __builtin_isfinite(((br + bg) + bb) + (b1 + b2));
		const float Np = took ? Nh : (COUNTS ? n : 1.0f);
		const float or_ = took ? br : cr, og = took ? bg : cg, ob = took ? bb : cb, m1 = took ? b1 : L, m2 = took ? b2 : LL;

		// 4. the variance the filter starts from
		const float vf = Np < (COUNTS ? 4.0f * n : 4.0f) ? v0 : fmaxf(0.0f, m2 - m1 * m1);
		const float var = vf * ((COUNTS ? n : 1.0f) / Np);

		// 5. the next frame's history, and the filter's state, guide and re-modulation record
		next.color[p] = make_float4(or_, og, ob, Np);
		next.moments[p] = make_float2(m1, m2);
		next.geometry[p] = g;
		if (col_var != nullptr) {
			col_var[p] = make_float4(or_, og, ob, var);
			guide[p] = g;
			remod[p] = make_float4(ax, ay, az, (A.w + B.w) / n);
		}
	}
	// the two counts of the wave in one atomic
	const uint64_t m_took = __ballot(took), m_reset = __ballot(inside && !took);
	if ((threadIdx.x & 63u) == 0u && (m_took | m_reset) != 0)
		atomicAdd(counter + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) % kTpCounterSlots) * kTpCounterStride,
		          (unsigned long long)__popcll(m_took) | ((unsigned long long)__popcll(m_reset) << 32));
}

namespace {
template <bool COUNTS, bool SEARCH, bool UNIT>
hipError_t tp_launch(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, const float4* motion, const TemporalHistory& prev,
                     const TemporalHistory& next, const TemporalParams& T, float4* col_var, float4* guide, float4* remod, unsigned long long* counter, hipStream_t stream) {
	const dim3 grid((T.W + kTpBlockX - 1) / kTpBlockX, (T.H + kTpBlockY - 1) / kTpBlockY), block(kTpBlockX, kTpBlockY);
	hipLaunchKernelGGL((k_tp_accumulate<COUNTS, SEARCH, UNIT>), grid, block, 0, stream, a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter);
	return hipGetLastError();
}
}  // namespace

hipError_t launch_temporal_accumulate(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, const float4* motion, const TemporalHistory& prev,
                                      const TemporalHistory& next, const TemporalParams& T, float4* col_var, float4* guide, float4* remod, unsigned long long* counter,
                                      hipStream_t stream) {
	return tp_launch<false, false, false>(a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter, stream);
}

hipError_t launch_temporal_accumulate_counts(const float4* a, const float4* b, const float4* albedo_cov, const float4* normal_depth, const float4* motion,
                                             const TemporalHistory& prev, const TemporalHistory& next, const TemporalParams& T, bool search, bool unit_normals, float4* col_var,
                                             float4* guide, float4* remod, unsigned long long* counter, hipStream_t stream) {
	if (search && unit_normals) return tp_launch<true, true, true>(a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter, stream);
	if (search) return tp_launch<true, true, false>(a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter, stream);
	if (unit_normals) return tp_launch<true, false, true>(a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter, stream);
	return tp_launch<true, false, false>(a, b, albedo_cov, normal_depth, motion, prev, next, T, col_var, guide, remod, counter, stream);
}

}  // namespace ptx
