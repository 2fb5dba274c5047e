// The batch entry points of the C ABI: ptx_denoise, ptx_denoise_counts and the two temporal calls, the adaptive decision, the mean of two half-frames, the kernels' unit-test batches
// (PBR, leaf intersection, exact math, camera rays, materials), the framebuffer reduction, tone mapping and PNG encoding.
#include <dlfcn.h>
#include <zlib.h>

#include <chrono>

#include "api_internal.hpp"

namespace {

// Which iterations (bit i = step 2^i) run the LDS-tiled a-trous kernel rather than the global gather: the faster of the two per step at
// 1920 x 1080 on the MI355X (profiles/EXPERIMENTS.md). PTX_DENOISE_TILED=<mask>: measurement switch. Both forms give the same bits.
constexpr uint32_t kDenoiseTiledSteps = 0x00;
uint32_t denoise_tiled_steps() {
	const char* e = getenv("PTX_DENOISE_TILED");
	return e && *e ? (uint32_t)strtoul(e, nullptr, 0) : kDenoiseTiledSteps;
}

// ptx_denoise and ptx_denoise_counts: the same refusals, workspace and kernels but for step 1 of the filter. counts = false: `spp_a` and `spp_b`
// are the halves' sample counts (k_dn_prepare); counts = true: the halves carry per-pixel counts in .w and `spp_a` is guide_spp (k_dn_prepare_counts).
struct DenoiseCall {
	const char* who;
	uint32_t W, H, iterations;
	float sigma_l, sigma_n, sigma_z;
	bool counts;
	uint32_t spp_a, spp_b;
};

// Steps 2 to 5 of the filter on a prepared state: state[0] holds (col, v0), guide and remod what step 1 left. What ptx_denoise,
// ptx_denoise_counts and ptx_denoise_temporal share after their own step 1. The caller holds the context's mutex.
int denoise_filter(ptx_ctx* c, uint32_t W, uint32_t H, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float4* const state[2], const float4* guide,
                   const float4* remod, float4* d_out) {
	const uint32_t tiled = denoise_tiled_steps();
	HIP_TRY(launch_denoise_prefilter(state[0], guide, W, H, sigma_n, sigma_z, state[1], c->stream));
	for (uint32_t i = 0; i < iterations; i++) {
		const bool last = i + 1 == iterations;
		const float4* in = state[(i + 1) & 1u];
		HIP_TRY(launch_denoise_atrous(in, guide, remod, W, H, 1u << i, sigma_l, sigma_n, sigma_z, last, (tiled >> i) & 1u, last ? d_out : state[i & 1u], c->stream));
	}
	return PTX_OK;
}

int denoise_frame(ptx_ctx* c, const DenoiseCall& D, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, float* out_rgba, ptx_denoise_stats* stats) {
	const std::string who = D.who;
	// every refusal below is decided before any device work
	if (!c || !accum_a || !accum_b || !guides || !out_rgba) return set_err(PTX_ERR_INVALID, who + ": NULL argument");
	if (!guides->albedo_cov || !guides->normal_depth) return set_err(PTX_ERR_INVALID, who + ": both guide buffers are required");
	if (!D.W || !D.H || D.W > 16384 || D.H > 16384) return set_err(PTX_ERR_INVALID, who + ": W and H must be in 1 .. 16384");
	if (D.counts && !D.spp_a) return set_err(PTX_ERR_INVALID, who + ": guide_spp must be > 0 (the samples of every pixel the guides hold)");
	if (!D.counts && (!D.spp_a || !D.spp_b)) return set_err(PTX_ERR_INVALID, who + ": spp_a and spp_b must be > 0 (the noise estimate needs two half-frames)");
	if (D.iterations > 8) return set_err(PTX_ERR_INVALID, who + ": at most 8 iterations");
	if (!(D.sigma_l >= 0.0f) || !(D.sigma_n >= 0.0f) || !(D.sigma_z >= 0.0f)) return set_err(PTX_ERR_INVALID, who + ": a sigma is negative or NaN");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev || is_device_ptr(guides->albedo_cov) != dev || is_device_ptr(guides->normal_depth) != dev || is_device_ptr(out_rgba) != dev)
		return set_err(PTX_ERR_INVALID, who + ": the five buffers must all be device or all be host memory");
	const uint32_t W = D.W, H = D.H, iterations = D.iterations ? D.iterations : 5u;
	const float sigma_l = D.sigma_l != 0.0f ? D.sigma_l : 4.0f, sigma_n = D.sigma_n != 0.0f ? D.sigma_n : 0.5f, sigma_z = D.sigma_z != 0.0f ? D.sigma_z : 0.1f;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_denoise_stats{};

	const size_t n = (size_t)W * H, bytes = n * sizeof(float4);
	const size_t ws_bytes = bytes * (dev ? 4 : 8);
	HIP_TRY(c->denoise.ensure(ws_bytes));
	float4* const ws = (float4*)c->denoise.p;
	float4 *const state[2] = {ws, ws + n}, *const guide = ws + 2 * n, *const remod = ws + 3 * n;
	// workspace: [state 0][state 1][guide][remod], then the staging of the four host inputs; the staged output takes accum_a's place:
	// prepare has consumed the inputs before the last iteration writes
	const void* const src[4] = {accum_a, accum_b, guides->albedo_cov, guides->normal_depth};
	Staged in[4], s_out;
	for (int k = 0; k < 4; k++) HIP_TRY(in[k].bind(c, dev, src[k], bytes, c->denoise, (4 + k) * bytes));
	HIP_TRY(s_out.bind(c, dev, out_rgba, bytes, c->denoise, 4 * bytes, kOutputOnly));
	float4* const d_out = s_out.as<float4>();
	if (stats)
		if (const int rc = PassFrame::ensure_events(c, 1); rc != PTX_OK) return rc;
	if (stats) HIP_TRY(hipEventRecord(c->events[0], c->stream));
	if (D.counts) HIP_TRY(launch_denoise_prepare_counts(in[0].as<float4>(), in[1].as<float4>(), in[2].as<float4>(), in[3].as<float4>(), D.spp_a, n, state[0], guide, remod, c->stream));
	else HIP_TRY(launch_denoise_prepare(in[0].as<float4>(), in[1].as<float4>(), in[2].as<float4>(), in[3].as<float4>(), D.spp_a, D.spp_b, n, state[0], guide, remod, c->stream));
	if (const int rc = denoise_filter(c, W, H, iterations, sigma_l, sigma_n, sigma_z, state, guide, remod, d_out); rc != PTX_OK) return rc;
	if (stats) HIP_TRY(hipEventRecord(c->events[1], c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (stats || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) {
		if (const int rc = PassFrame::pass_ms(c, 1, &stats->kernel_ms); rc != PTX_OK) return rc;
		stats->iterations = iterations;
		stats->workspace_bytes = ws_bytes;
	}
	return PTX_OK;
}

}  // namespace

int ptx_denoise(ptx_ctx* c, const ptx_denoise_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, float* out_rgba, ptx_denoise_stats* stats) {
	if (!cfg) return set_err(PTX_ERR_INVALID, "ptx_denoise: NULL argument");
	return denoise_frame(c, DenoiseCall{"ptx_denoise", cfg->W, cfg->H, cfg->iterations, cfg->sigma_l, cfg->sigma_n, cfg->sigma_z, false, cfg->spp_a, cfg->spp_b}, accum_a, accum_b, guides,
	                     out_rgba, stats);
}

int ptx_denoise_counts(ptx_ctx* c, const ptx_denoise_counts_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, float* out_rgba,
                       ptx_denoise_stats* stats) {
	if (!cfg) return set_err(PTX_ERR_INVALID, "ptx_denoise_counts: NULL argument");
	return denoise_frame(c, DenoiseCall{"ptx_denoise_counts", cfg->W, cfg->H, cfg->iterations, cfg->sigma_l, cfg->sigma_n, cfg->sigma_z, true, cfg->guide_spp, 0u}, accum_a, accum_b,
	                     guides, out_rgba, stats);
}

namespace {

// ptx_denoise_temporal and ptx_denoise_temporal_counts: the same refusals, workspace, staging and counters; they differ in step 1 and the
// blend of the accumulation kernel. counts = false: spp_a, spp_b are the halves' sample counts and max_history counts frames; counts = true:
// the halves carry per-pixel counts in .w, spp_a is guide_spp, max_history counts samples and flags are the PTX_TEMPORAL_* bits.
struct TemporalCall {
	const char* who;
	uint32_t W, H, iterations;
	float sigma_l, sigma_n, sigma_z;
	bool counts;
	uint32_t spp_a, spp_b, max_history;
	float tau_z, tau_n;
	uint32_t flags;
};

int temporal_frame(ptx_ctx* c, const TemporalCall* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, const float* motion,
                   const ptx_temporal_history* prev, const ptx_temporal_history* next, float* out_rgba, ptx_temporal_stats* stats) {
	const std::string who = cfg->who;
	// every refusal below is decided before any device work; the context comes last of the arguments, so that a caller without a GPU meets
	// every other refusal first
	if (!accum_a || !accum_b || !guides || !motion || !next) return set_err(PTX_ERR_INVALID, who + ": NULL argument");
	if (!guides->albedo_cov || !guides->normal_depth) return set_err(PTX_ERR_INVALID, who + ": both guide buffers are required");
	if (!next->color || !next->moments || !next->geometry) return set_err(PTX_ERR_INVALID, who + ": a member of next is NULL");
	if (prev && (!prev->color || !prev->moments || !prev->geometry)) return set_err(PTX_ERR_INVALID, who + ": a member of prev is NULL (pass prev = NULL for the first frame)");
	if (prev) {
		const float* const np[3] = {next->color, next->moments, next->geometry};
		const float* const pp[3] = {prev->color, prev->moments, prev->geometry};
		for (const float* a : np)
			for (const float* b : pp)
				if (a == b) return set_err(PTX_ERR_INVALID, who + ": next shares a buffer with prev (neighbouring pixels of prev are read while next is written)");
	}
	if (!cfg->W || !cfg->H || cfg->W > 16384 || cfg->H > 16384) return set_err(PTX_ERR_INVALID, who + ": W and H must be in 1 .. 16384");
	if (cfg->counts && !cfg->spp_a) return set_err(PTX_ERR_INVALID, who + ": guide_spp must be > 0 (the samples of every pixel the guides and the motion hold)");
	if (!cfg->counts && (!cfg->spp_a || !cfg->spp_b)) return set_err(PTX_ERR_INVALID, who + ": spp_a and spp_b must be > 0 (the noise estimate needs two half-frames)");
	if (cfg->iterations > 8) return set_err(PTX_ERR_INVALID, who + ": at most 8 iterations");
	if (!(cfg->sigma_l >= 0.0f) || !(cfg->sigma_n >= 0.0f) || !(cfg->sigma_z >= 0.0f)) return set_err(PTX_ERR_INVALID, who + ": a sigma is negative or NaN");
	if (cfg->counts && cfg->max_history > 1048576) return set_err(PTX_ERR_INVALID, who + ": max_history above 1048576 samples");
	if (!cfg->counts && cfg->max_history > 1024) return set_err(PTX_ERR_INVALID, who + ": max_history above 1024");
	if (!(cfg->tau_z >= 0.0f) || !(cfg->tau_n >= 0.0f)) return set_err(PTX_ERR_INVALID, who + ": a tau is negative or NaN");
	if (cfg->flags & ~(PTX_TEMPORAL_SEARCH_3X3 | PTX_TEMPORAL_UNIT_NORMALS)) return set_err(PTX_ERR_INVALID, who + ": unknown bit in flags");
	if (!c) return set_err(PTX_ERR_INVALID, who + ": NULL context");
	const bool dev = is_device_ptr(accum_a);
	{
		const void* all[12] = {accum_b, guides->albedo_cov, guides->normal_depth, motion, next->color, next->moments, next->geometry, prev ? prev->color : nullptr,
		                       prev ? prev->moments : nullptr, prev ? prev->geometry : nullptr, out_rgba, nullptr};
		for (const void* p : all)
			if (p && is_device_ptr(p) != dev) return set_err(PTX_ERR_INVALID, who + ": the buffers must all be device or all be host memory");
	}
	const uint32_t W = cfg->W, H = cfg->H, iterations = cfg->iterations ? cfg->iterations : 5u;
	const float sigma_l = cfg->sigma_l != 0.0f ? cfg->sigma_l : 4.0f, sigma_n = cfg->sigma_n != 0.0f ? cfg->sigma_n : 0.5f, sigma_z = cfg->sigma_z != 0.0f ? cfg->sigma_z : 0.1f;
	TemporalParams T{};
	T.W = (int)W; T.H = (int)H;
	if (cfg->counts) {   // n = float(guide_spp); the history is counted in samples
		T.n = (float)cfg->spp_a;
		T.max_history = (float)(cfg->max_history ? cfg->max_history : (uint32_t)std::min<uint64_t>(32ull * cfg->spp_a, 1048576ull));
	} else {
		T.n = (float)(cfg->spp_a + cfg->spp_b); T.na = (float)cfg->spp_a; T.nb = (float)cfg->spp_b;
		T.max_history = (float)(cfg->max_history ? cfg->max_history : 32u);
	}
	T.tau_z = cfg->tau_z != 0.0f ? cfg->tau_z : 0.1f;
	T.tau_n = cfg->tau_n != 0.0f ? cfg->tau_n : 0.9f;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_temporal_stats{};

	// workspace: [state 0][state 1][guide][remod][counter slots], then the staging of host buffers: the five inputs, prev, next and the output
	const size_t n = (size_t)W * H, b16 = n * sizeof(float4), b8 = n * sizeof(float2);
	const size_t o_counter = 4 * b16, o_stage = o_counter + kTpCounterBytes;
	const size_t ws_bytes = dev ? o_stage : o_stage + 5 * b16 + 2 * (2 * b16 + pad16(b8)) + b16;
	HIP_TRY(c->denoise.ensure(ws_bytes));
	float4* const ws = (float4*)c->denoise.p;
	float4 *const state[2] = {ws, ws + n}, *const guide = ws + 2 * n, *const remod = ws + 3 * n;
	unsigned long long* const counter = (unsigned long long*)((char*)c->denoise.p + o_counter);
	size_t off = o_stage;
	auto stage = [&](Staged& s, const void* p, size_t bytes, bool copy_in) {
		const hipError_t e = s.bind(c, dev, p, bytes, c->denoise, off, copy_in);
		off += pad16(bytes);   // an odd pixel count leaves the moments 8 bytes short of a float4 boundary
		return e;
	};
	const void* const src[5] = {accum_a, accum_b, guides->albedo_cov, guides->normal_depth, motion};
	Staged in[5], s_prev[3], s_next[3], s_out;
	for (int k = 0; k < 5; k++) HIP_TRY(stage(in[k], src[k], b16, true));
	const size_t hist_bytes[3] = {b16, b8, b16};
	const void* const pp[3] = {prev ? prev->color : nullptr, prev ? prev->moments : nullptr, prev ? prev->geometry : nullptr};
	const void* const np[3] = {next->color, next->moments, next->geometry};
	for (int k = 0; k < 3; k++) {
		if (prev) HIP_TRY(stage(s_prev[k], pp[k], hist_bytes[k], true));
		else off += pad16(hist_bytes[k]);
	}
	for (int k = 0; k < 3; k++) HIP_TRY(stage(s_next[k], np[k], hist_bytes[k], kOutputOnly));
	if (out_rgba) HIP_TRY(stage(s_out, out_rgba, b16, kOutputOnly));
	const TemporalHistory d_prev{s_prev[0].as<float4>(), s_prev[1].as<float2>(), s_prev[2].as<float4>()};   // all nullptr without prev
	const TemporalHistory d_next{s_next[0].as<float4>(), s_next[1].as<float2>(), s_next[2].as<float4>()};
	if (stats)
		if (const int rc = PassFrame::ensure_events(c, 2); rc != PTX_OK) return rc;
	HIP_TRY(hipMemsetAsync(counter, 0, kTpCounterBytes, c->stream));
	if (stats) HIP_TRY(hipEventRecord(c->events[0], c->stream));
	if (cfg->counts)
		HIP_TRY(launch_temporal_accumulate_counts(in[0].as<float4>(), in[1].as<float4>(), in[2].as<float4>(), in[3].as<float4>(), in[4].as<float4>(), d_prev, d_next, T,
		                                          (cfg->flags & PTX_TEMPORAL_SEARCH_3X3) != 0, (cfg->flags & PTX_TEMPORAL_UNIT_NORMALS) != 0, out_rgba ? state[0] : nullptr, guide,
		                                          remod, counter, c->stream));
	else
		HIP_TRY(launch_temporal_accumulate(in[0].as<float4>(), in[1].as<float4>(), in[2].as<float4>(), in[3].as<float4>(), in[4].as<float4>(), d_prev, d_next, T,
		                                   out_rgba ? state[0] : nullptr, guide, remod, counter, c->stream));
	if (stats) HIP_TRY(hipEventRecord(c->events[1], c->stream));   // the end of the accumulation and the start of the filter
	if (out_rgba)
		if (const int rc = denoise_filter(c, W, H, iterations, sigma_l, sigma_n, sigma_z, state, guide, remod, s_out.as<float4>()); rc != PTX_OK) return rc;
	if (stats) HIP_TRY(hipEventRecord(c->events[2], c->stream));
	for (const Staged& s : s_next) HIP_TRY(s.copy_back(c));
	HIP_TRY(s_out.copy_back(c));
	std::vector<unsigned long long> slots;
	if (stats) {
		slots.resize(kTpCounterSlots * kTpCounterStride);
		HIP_TRY(hipMemcpyAsync(slots.data(), counter, kTpCounterBytes, hipMemcpyDeviceToHost, c->stream));
	}
	if (stats || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) {
		float t = 0;
		HIP_TRY(hipEventElapsedTime(&t, c->events[0], c->events[1]));
		stats->accumulate_ms = t;
		if (out_rgba) {
			HIP_TRY(hipEventElapsedTime(&t, c->events[1], c->events[2]));
			stats->filter.kernel_ms = t;
			stats->filter.iterations = iterations;
		}
		stats->filter.workspace_bytes = ws_bytes;
		for (uint32_t k = 0; k < kTpCounterSlots; k++) {
			stats->reprojected += slots[(size_t)k * kTpCounterStride] & 0xFFFFFFFFull;
			stats->reset += slots[(size_t)k * kTpCounterStride] >> 32;
		}
	}
	return PTX_OK;
}

}  // namespace

int ptx_denoise_temporal(ptx_ctx* c, const ptx_temporal_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, const float* motion,
                         const ptx_temporal_history* prev, const ptx_temporal_history* next, float* out_rgba, ptx_temporal_stats* stats) {
	if (!cfg) return set_err(PTX_ERR_INVALID, "ptx_denoise_temporal: NULL argument");
	const TemporalCall call{"ptx_denoise_temporal", cfg->W, cfg->H, cfg->iterations, cfg->sigma_l, cfg->sigma_n, cfg->sigma_z, false, cfg->spp_a, cfg->spp_b, cfg->max_history,
	                        cfg->tau_z, cfg->tau_n, 0u};
	return temporal_frame(c, &call, accum_a, accum_b, guides, motion, prev, next, out_rgba, stats);
}

int ptx_denoise_temporal_counts(ptx_ctx* c, const ptx_temporal_counts_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, const float* motion,
                                const ptx_temporal_history* prev, const ptx_temporal_history* next, float* out_rgba, ptx_temporal_stats* stats) {
	if (!cfg) return set_err(PTX_ERR_INVALID, "ptx_denoise_temporal_counts: NULL argument");
	const TemporalCall call{"ptx_denoise_temporal_counts", cfg->W, cfg->H, cfg->iterations, cfg->sigma_l, cfg->sigma_n, cfg->sigma_z, true, cfg->guide_spp, 0u, cfg->max_history,
	                        cfg->tau_z, cfg->tau_n, cfg->flags};
	return temporal_frame(c, &call, accum_a, accum_b, guides, motion, prev, next, out_rgba, stats);
}

namespace {

// the decision's workspace on the context, laid out for a w x h rectangle; tile_count_all: the sharded decision's second count per tile
int adaptive_workspace(ptx_ctx* c, uint32_t w, uint32_t h, AdaptiveBuffers& B, uint32_t*& tile_count_all) {
	const size_t n = (size_t)w * h, tiles = (size_t)((w + kAdTile - 1) / kAdTile) * ((h + kAdTile - 1) / kAdTile), blocks = tiles * kAdBlocksPerTile;
	const size_t o_mask = pad16(n), o_boff = o_mask + blocks * 8, o_tcnt = o_boff + blocks * 4, o_toff = o_tcnt + pad16(tiles * 4), o_cnt = o_toff + pad16(tiles * 4);
	const size_t o_tall = o_cnt + 16;
	HIP_TRY(c->adaptive.ensure(o_tall + pad16(tiles * 4)));
	char* const ws = (char*)c->adaptive.p;
	B = AdaptiveBuffers{(uint8_t*)ws, (unsigned long long*)(ws + o_mask), (uint32_t*)(ws + o_boff), (uint32_t*)(ws + o_tcnt), (uint32_t*)(ws + o_toff), (uint32_t*)(ws + o_cnt)};
	tile_count_all = (uint32_t*)(ws + o_tall);
	return PTX_OK;
}

int adaptive_events(ptx_ctx* c) {
	for (hipEvent_t& ev : c->adaptive_ev)
		if (!ev) HIP_TRY(hipEventCreate(&ev));
	return PTX_OK;
}

// adds the time between the two events to *select_ms; the stream is synchronised
int adaptive_elapsed(ptx_ctx* c, double* select_ms) {
	float t = 0;
	HIP_TRY(hipEventElapsedTime(&t, c->adaptive_ev[0], c->adaptive_ev[1]));
	*select_ms += t;
	return PTX_OK;
}

}  // namespace

int adaptive_decide_locked(ptx_ctx* c, uint32_t w, uint32_t h, const float4* d_a, const float4* d_b, float threshold, uint8_t* d_done, uint32_t* d_pixels, uint32_t& n_active,
                           double* select_ms) {
	AdaptiveBuffers B{};
	uint32_t* unused = nullptr;
	if (const int rc = adaptive_workspace(c, w, h, B, unused); rc != PTX_OK) return rc;
	if (select_ms)
		if (const int rc = adaptive_events(c); rc != PTX_OK) return rc;
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[0], c->stream));
	HIP_TRY(launch_adaptive_select(d_a, d_b, w, h, threshold, B, d_done, d_pixels, c->stream));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[1], c->stream));
	HIP_TRY(hipMemcpyAsync(&n_active, B.n_active, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (select_ms) return adaptive_elapsed(c, select_ms);
	return PTX_OK;
}

int adaptive_decide_sharded_locked(ptx_ctx* c, uint32_t w, uint32_t h, const AdaptiveShard& shard, bool mask_on_device, const float4* d_a, const float4* d_b, float threshold,
                                   uint8_t* d_done, uint32_t* d_pixels, uint32_t& n_own, uint32_t& n_all, double* select_ms, bool& exchange_failed) {
	exchange_failed = false;
	ptx_ctx::MaskExchange& X = c->mask_exchange;
	const size_t n = (size_t)w * h;
	AdaptiveBuffers B{};
	uint32_t* tile_count_all = nullptr;
	if (const int rc = adaptive_workspace(c, w, h, B, tile_count_all); rc != PTX_OK) return rc;
	if (select_ms)
		if (const int rc = adaptive_events(c); rc != PTX_OK) return rc;
	// a device mask is written and read where the caller keeps it; a host one goes through the workspace's noisy bytes
	uint8_t* const d_mask = mask_on_device ? X.mask : B.noisy;
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[0], c->stream));
	HIP_TRY(launch_adaptive_noisy_shard(d_a, d_b, w, h, threshold, shard, d_mask, c->stream));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[1], c->stream));
	if (!mask_on_device) HIP_TRY(hipMemcpyAsync(X.mask, d_mask, n, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (select_ms)
		if (const int rc = adaptive_elapsed(c, select_ms); rc != PTX_OK) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	const int status = X.fn(X.user, X.mask, n);
	X.wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	X.calls++;
	if (status != 0) {
		exchange_failed = true;
		return set_err(PTX_ERR_HIP, "mask exchange failed (status " + std::to_string(status) + ")");
	}
	if (!mask_on_device) HIP_TRY(hipMemcpyAsync(d_mask, X.mask, n, hipMemcpyHostToDevice, c->stream));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[0], c->stream));
	HIP_TRY(launch_adaptive_decide_shard(d_mask, w, h, shard, B, tile_count_all, d_done, d_pixels, c->stream));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[1], c->stream));
	uint32_t counts[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(counts, B.n_active, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	n_own = counts[0];
	n_all = counts[1];
	if (select_ms) return adaptive_elapsed(c, select_ms);
	return PTX_OK;
}

int ptx_ctx_set_mask_exchange(ptx_ctx* c, ptx_mask_exchange_fn fn, void* user, uint8_t* mask, size_t mask_bytes) {
	if (!c) return set_err(PTX_ERR_INVALID, "ptx_ctx_set_mask_exchange: NULL context");
	if (fn && !mask) return set_err(PTX_ERR_INVALID, "ptx_ctx_set_mask_exchange: a callback needs a mask buffer");
	std::lock_guard<std::mutex> lk(c->mu);
	ptx_ctx::MaskExchange& X = c->mask_exchange;
	X.fn = fn;
	X.user = fn ? user : nullptr;
	X.mask = fn ? mask : nullptr;
	X.bytes = fn ? mask_bytes : 0;
	return PTX_OK;
}

int ptx_ctx_get_mask_exchange_stats(ptx_ctx* c, uint64_t* calls, double* wall_ms) {
	if (!c) return set_err(PTX_ERR_INVALID, "ptx_ctx_get_mask_exchange_stats: NULL context");
	std::lock_guard<std::mutex> lk(c->mu);
	if (calls) *calls = c->mask_exchange.calls;
	if (wall_ms) *wall_ms = c->mask_exchange.wall_ms;
	return PTX_OK;
}

int ptx_adaptive_select(ptx_ctx* c, uint32_t w, uint32_t h, const float* accum_a, const float* accum_b, float threshold, uint8_t* done, uint32_t* pixels, uint32_t* n_active) {
	// every refusal below is decided before any device work
	if (!c || !accum_a || !accum_b || !done || !n_active) return set_err(PTX_ERR_INVALID, "ptx_adaptive_select: NULL argument");
	if (!w || !h || w > kAdMaxSide || h > kAdMaxSide) return set_err(PTX_ERR_INVALID, "ptx_adaptive_select: w and h must be in 1 .. 16384");
	if (!(threshold >= 0.0f)) return set_err(PTX_ERR_INVALID, "ptx_adaptive_select: threshold is negative or NaN");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev || is_device_ptr(done) != dev || (pixels && is_device_ptr(pixels) != dev))
		return set_err(PTX_ERR_INVALID, "ptx_adaptive_select: the buffers must all be device or all be host memory");
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)w * h, bytes = n * sizeof(float4);
	Staged s_a, s_b, s_done, s_pixels;
	if (!dev) {
		HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
		HIP_TRY(c->adaptive_state.ensure(n * 4 + pad16(n)));
	}
	HIP_TRY(s_a.bind(c, dev, accum_a, bytes, c->adaptive_stage));
	HIP_TRY(s_b.bind(c, dev, accum_b, bytes, c->adaptive_stage, bytes));
	if (pixels) HIP_TRY(s_pixels.bind(c, dev, pixels, n * 4, c->adaptive_state, 0, kOutputOnly));
	HIP_TRY(s_done.bind(c, dev, done, n, c->adaptive_state, n * 4));
	uint32_t count = 0;
	if (const int rc = adaptive_decide_locked(c, w, h, s_a.as<float4>(), s_b.as<float4>(), threshold, s_done.as<uint8_t>(), s_pixels.as<uint32_t>(), count, nullptr); rc != PTX_OK) return rc;
	HIP_TRY(s_done.copy_back(c));
	if (count) HIP_TRY(s_pixels.copy_back(c, (size_t)count * 4));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	*n_active = count;
	return PTX_OK;
}

int ptx_accum_mean(ptx_ctx* c, const float* accum_a, const float* accum_b, size_t n_pixels, float* out_rgba) {
	if (!c || !accum_a || !out_rgba) return set_err(PTX_ERR_INVALID, "ptx_accum_mean: NULL argument");
	if (n_pixels > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_accum_mean: buffer too large");
	const bool dev = is_device_ptr(accum_a);
	if ((accum_b && is_device_ptr(accum_b) != dev) || is_device_ptr(out_rgba) != dev)
		return set_err(PTX_ERR_INVALID, "ptx_accum_mean: the buffers must all be device or all be host memory");
	if (n_pixels == 0) return PTX_OK;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t bytes = n_pixels * sizeof(float4);
	Staged s_a, s_b, s_out;   // the staged output is written over the staged accum_a
	if (!dev) HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
	HIP_TRY(s_a.bind(c, dev, accum_a, bytes, c->adaptive_stage));
	if (accum_b) HIP_TRY(s_b.bind(c, dev, accum_b, bytes, c->adaptive_stage, bytes));
	HIP_TRY(s_out.bind(c, dev, out_rgba, bytes, c->adaptive_stage, 0, kOutputOnly));
	HIP_TRY(launch_accum_mean(s_a.as<float4>(), s_b.as<float4>(), n_pixels, s_out.as<float4>(), c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

namespace {

// What ptx_emission_split and ptx_emission_merge refuse, in one order, before any device work; the context is looked at last. `x`, `y`: the
// buffers worked on in place (y may be NULL). -> whether they are device memory.
int emission_args(const char* who_c, const ptx_ctx* c, const float* emission, uint32_t guide_spp, size_t n_pixels, const float* x, const float* y, bool& dev) {
	const std::string who = who_c;
	if (!emission || !x) return set_err(PTX_ERR_INVALID, who + ": NULL argument");
	if (guide_spp == 0) return set_err(PTX_ERR_INVALID, who + ": guide_spp must be > 0");
	if (n_pixels == 0 || n_pixels > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, who + ": n_pixels must lie in 1 .. 2^31 - 1");
	if (emission == x || emission == y || x == y) return set_err(PTX_ERR_INVALID, who + ": a buffer shares its memory with another");
	if (!c) return set_err(PTX_ERR_INVALID, who + ": NULL context");
	dev = is_device_ptr(emission);
	if (is_device_ptr(x) != dev || (y && is_device_ptr(y) != dev)) return set_err(PTX_ERR_INVALID, who + ": the buffers must all be device or all be host memory");
	return PTX_OK;
}

}  // namespace

int ptx_emission_split(ptx_ctx* c, const float* emission, uint32_t guide_spp, size_t n_pixels, float* accum_a, float* accum_b) {
	bool dev = false;
	if (const int rc = emission_args("ptx_emission_split", c, emission, guide_spp, n_pixels, accum_a, accum_b, dev); rc != PTX_OK) return rc;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t bytes = n_pixels * sizeof(float4);
	Staged s_e, s_a, s_b;
	if (!dev) HIP_TRY(c->adaptive_stage.ensure(3 * bytes));
	HIP_TRY(s_e.bind(c, dev, emission, bytes, c->adaptive_stage));
	HIP_TRY(s_a.bind(c, dev, accum_a, bytes, c->adaptive_stage, bytes));
	if (accum_b) HIP_TRY(s_b.bind(c, dev, accum_b, bytes, c->adaptive_stage, 2 * bytes));
	HIP_TRY(launch_emission_split(s_e.as<float4>(), guide_spp, n_pixels, s_a.as<float4>(), s_b.as<float4>(), c->stream));
	HIP_TRY(s_a.copy_back(c));
	HIP_TRY(s_b.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_emission_merge(ptx_ctx* c, const float* emission, uint32_t guide_spp, size_t n_pixels, float* out_rgba) {
	bool dev = false;
	if (const int rc = emission_args("ptx_emission_merge", c, emission, guide_spp, n_pixels, out_rgba, nullptr, dev); rc != PTX_OK) return rc;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t bytes = n_pixels * sizeof(float4);
	Staged s_e, s_out;
	if (!dev) HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
	HIP_TRY(s_e.bind(c, dev, emission, bytes, c->adaptive_stage));
	HIP_TRY(s_out.bind(c, dev, out_rgba, bytes, c->adaptive_stage, bytes));
	HIP_TRY(launch_emission_merge(s_e.as<float4>(), guide_spp, n_pixels, s_out.as<float4>(), c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_pbr_eval_batch(ptx_ctx* c, const float* in, size_t n, float* out) {
	if (!c) return set_err(PTX_ERR_NO_DEVICE, "ptx_pbr_eval_batch: no GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!in || !out) return set_err(PTX_ERR_INVALID, "ptx_pbr_eval_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_pbr_eval_batch: batch too large");
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(in);
	if (dev != is_device_ptr(out)) return set_err(PTX_ERR_INVALID, "ptx_pbr_eval_batch: in and out must both be device or both be host memory");
	Staged s_in, s_out;
	HIP_TRY(s_in.bind(c, dev, in, n * 14 * 4, c->stage_a));
	HIP_TRY(s_out.bind(c, dev, out, n * 15 * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(launch_pbr_eval(s_in.as<float>(), s_out.as<float>(), n, c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_leaf_intersect_batch(ptx_ctx* c, const float* corners, uint32_t n_tri, const uint32_t* refs, int leaf_ordered, const float* rays, size_t n,
                             float* out, int32_t* tri) {
	if (!c) return set_err(PTX_ERR_NO_DEVICE, "ptx_leaf_intersect_batch: no GPU context (no CPU path exists)");
	if (n_tri == 0 || n_tri > kLeafBatchMaxTris) return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: n_tri must be 1 .. 256");
	if (!corners) return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: NULL argument");
	if (n == 0) return PTX_OK;
	if (!rays || !out || !tri) return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF / 7) return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: batch too large");
	if (is_device_ptr(corners) || is_device_ptr(rays) || is_device_ptr(out) || is_device_ptr(tri) || (refs && is_device_ptr(refs)))
		return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: host memory only");
	std::vector<uint32_t> order(n_tri);
	std::vector<uint8_t> seen(n_tri, 0);
	for (uint32_t k = 0; k < n_tri; k++) {
		order[k] = refs ? refs[k] : k;
		if (order[k] >= n_tri || seen[order[k]]) return set_err(PTX_ERR_INVALID, "ptx_leaf_intersect_batch: refs is not a permutation of 0 .. n_tri-1");
		seen[order[k]] = 1;
	}
	// the records the builder makes for these triangles (ids = their indices), laid out as upload_scene lays out the two copies
	std::vector<TriIsect> recs(n_tri);
	for (uint32_t k = 0; k < n_tri; k++) {
		const uint32_t t = leaf_ordered ? order[k] : k;
		recs[k] = make_tri_isect(corners + 9 * (size_t)t, corners + 9 * (size_t)t + 3, corners + 9 * (size_t)t + 6, t);
	}
	const KdNode node[2] = {kd_make_leaf(0, n_tri), {0, 0}};
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t refs_off = 16, recs_off = refs_off + pad16((size_t)n_tri * 4), rays_off = recs_off + (size_t)n_tri * 48;
	HIP_TRY(c->stage_a.ensure(rays_off + n * 28));
	HIP_TRY(c->stage_b.ensure(n * 16));
	char* in = (char*)c->stage_a.p;
	HIP_TRY(hipMemcpyAsync(in, node, 16, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(in + refs_off, order.data(), (size_t)n_tri * 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(in + recs_off, recs.data(), (size_t)n_tri * 48, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(in + rays_off, rays, n * 28, hipMemcpyHostToDevice, c->stream));
	const int grid = (int)std::min<size_t>((size_t)c->n_cu, (n + 255) / 256);
	HIP_TRY(c->spill.ensure((size_t)c->n_cu * 4 * (size_t)kSpillWords * sizeof(uint2)));
	float* d_out = (float*)c->stage_b.p;
	int32_t* d_tri = (int32_t*)(d_out + 3 * n);
	HIP_TRY(launch_leaf_intersect((const uint2*)in, (const uint32_t*)(in + refs_off), (const float4*)(in + recs_off), n_tri, leaf_ordered == 0 ? 0u : (leaf_ordered == 2 ? 2u : 1u),
	                              (const float*)(in + rays_off), n, d_out, d_tri, (uint2*)c->spill.p, grid, c->stream));
	HIP_TRY(hipMemcpyAsync(out, d_out, n * 12, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(tri, d_tri, n * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));   // the staged vectors are locals
	return PTX_OK;
}

int ptx_exact_math_check(ptx_ctx* c, uint64_t* mismatches) {
	if (!c) return set_err(PTX_ERR_NO_DEVICE, "ptx_exact_math_check: no GPU context (no CPU path exists)");
	if (!mismatches) return set_err(PTX_ERR_INVALID, "ptx_exact_math_check: NULL argument");
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	HIP_TRY(c->stage_b.ensure(kExactMathForms * 8));
	HIP_TRY(hipMemsetAsync(c->stage_b.p, 0, kExactMathForms * 8, c->stream));
	HIP_TRY(launch_exact_math_check((unsigned long long*)c->stage_b.p, c->stream));
	HIP_TRY(hipMemcpyAsync(mismatches, c->stage_b.p, kExactMathForms * 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_shade_consts_check(ptx_ctx* c, const float* materials, size_t n, uint64_t* mismatches) {
	if (!c) return set_err(PTX_ERR_NO_DEVICE, "ptx_shade_consts_check: no GPU context (no CPU path exists)");
	if (!mismatches || (n && !materials)) return set_err(PTX_ERR_INVALID, "ptx_shade_consts_check: NULL argument");
	if (n > (size_t)1 << 24) return set_err(PTX_ERR_INVALID, "ptx_shade_consts_check: batch too large");
	if (n && is_device_ptr(materials)) return set_err(PTX_ERR_INVALID, "ptx_shade_consts_check: host memory only");
	*mismatches = 0;
	if (n == 0) return PTX_OK;
	std::vector<ShadeRec> recs(n, ShadeRec{});
	for (size_t k = 0; k < n; k++) {
		recs[k].mat.roughness = materials[9 * k];
		recs[k].mat.ior = materials[9 * k + 2];
		fill_shade_consts(recs[k]);
	}
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t rec_off = pad16(n * 36);
	HIP_TRY(c->stage_a.ensure(rec_off + n * sizeof(ShadeRec)));
	HIP_TRY(c->stage_b.ensure(8));
	char* in = (char*)c->stage_a.p;
	HIP_TRY(hipMemcpyAsync(in, materials, n * 36, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(in + rec_off, recs.data(), n * sizeof(ShadeRec), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemsetAsync(c->stage_b.p, 0, 8, c->stream));
	HIP_TRY(launch_shade_consts_check((const float*)in, (const ShadeRec*)(in + rec_off), n, (unsigned long long*)c->stage_b.p, c->stream));
	HIP_TRY(hipMemcpyAsync(mismatches, c->stage_b.p, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));   // the staged records are locals
	return PTX_OK;
}

int ptx_camera_rays_batch(ptx_scene* sc, const float* ndc_ratio, size_t n, float* rays) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_camera_rays_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_camera_rays_batch: scene was created without a GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!ndc_ratio || !rays) return set_err(PTX_ERR_INVALID, "ptx_camera_rays_batch: NULL argument");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(ndc_ratio);
	if (dev != is_device_ptr(rays)) return set_err(PTX_ERR_INVALID, "ptx_camera_rays_batch: in and out must both be device or both be host memory");
	Staged s_in, s_out;
	HIP_TRY(s_in.bind(c, dev, ndc_ratio, n * 3 * 4, c->stage_a));
	HIP_TRY(s_out.bind(c, dev, rays, n * 6 * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(launch_camera_rays(sc->dev, s_in.as<float>(), s_out.as<float>(), n, c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_camera_lens_rays_batch(ptx_scene* sc, const float* in, size_t n, float* rays) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_camera_lens_rays_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_camera_lens_rays_batch: scene was created without a GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!in || !rays) return set_err(PTX_ERR_INVALID, "ptx_camera_lens_rays_batch: NULL argument");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(in);
	if (dev != is_device_ptr(rays)) return set_err(PTX_ERR_INVALID, "ptx_camera_lens_rays_batch: in and out must both be device or both be host memory");
	Staged s_in, s_out;
	HIP_TRY(s_in.bind(c, dev, in, n * 5 * 4, c->stage_a));
	HIP_TRY(s_out.bind(c, dev, rays, n * 6 * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(launch_camera_lens_rays(sc->dev, s_in.as<float>(), s_out.as<float>(), n, c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_punctual_pick_batch(ptx_scene* sc, const float* pos_u, size_t n, int32_t* light, float* pmf) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_punctual_pick_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_punctual_pick_batch: scene was created without a GPU context (no CPU path exists)");
	if (n && (!pos_u || !light || !pmf)) return set_err(PTX_ERR_INVALID, "ptx_punctual_pick_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_punctual_pick_batch: batch too large");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	NeePunctual Pn{};
	if (const int rc = punctual_on_device_locked(sc, Pn); rc != PTX_OK) return rc;
	if (Pn.n == 0) return set_err(PTX_ERR_INVALID, "ptx_punctual_pick_batch: the scene has no punctual lights");
	if (n == 0) return PTX_OK;
	const bool dev = is_device_ptr(pos_u);
	if (dev != is_device_ptr(light) || dev != is_device_ptr(pmf))
		return set_err(PTX_ERR_INVALID, "ptx_punctual_pick_batch: pos_u, light and pmf must all be device or all be host memory");
	Staged s_in, s_light, s_pmf;   // light and pmf share stage_b
	if (!dev) HIP_TRY(c->stage_b.ensure(n * 8));
	HIP_TRY(s_in.bind(c, dev, pos_u, n * 16, c->stage_a));
	HIP_TRY(s_light.bind(c, dev, light, n * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(s_pmf.bind(c, dev, pmf, n * 4, c->stage_b, n * 4, kOutputOnly));
	HIP_TRY(launch_punctual_pick(Pn, s_in.as<float>(), n, s_light.as<int32_t>(), s_pmf.as<float>(), c->stream));
	HIP_TRY(s_light.copy_back(c));
	HIP_TRY(s_pmf.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_light_pick_batch(ptx_scene* sc, const float* pos_u, size_t n, int32_t* light, float* pmf) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_light_pick_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_light_pick_batch: scene was created without a GPU context (no CPU path exists)");
	if (n && (!pos_u || !light || !pmf)) return set_err(PTX_ERR_INVALID, "ptx_light_pick_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_light_pick_batch: batch too large");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	NeeLights Lt{};
	if (const int rc = lights_on_device_locked(sc, Lt); rc != PTX_OK) return rc;
	if (Lt.n == 0) return set_err(PTX_ERR_INVALID, "ptx_light_pick_batch: the scene's light list is empty");
	if (n == 0) return PTX_OK;
	const bool dev = is_device_ptr(pos_u);
	if (dev != is_device_ptr(light) || dev != is_device_ptr(pmf))
		return set_err(PTX_ERR_INVALID, "ptx_light_pick_batch: pos_u, light and pmf must all be device or all be host memory");
	Staged s_in, s_light, s_pmf;   // light and pmf share stage_b
	if (!dev) HIP_TRY(c->stage_b.ensure(n * 8));
	HIP_TRY(s_in.bind(c, dev, pos_u, n * 16, c->stage_a));
	HIP_TRY(s_light.bind(c, dev, light, n * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(s_pmf.bind(c, dev, pmf, n * 4, c->stage_b, n * 4, kOutputOnly));
	HIP_TRY(launch_light_pick(Lt, s_in.as<float>(), n, s_light.as<int32_t>(), s_pmf.as<float>(), c->stream));
	HIP_TRY(s_light.copy_back(c));
	HIP_TRY(s_pmf.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_light_pmf_batch(ptx_scene* sc, const float* pos, const int32_t* light, size_t n, float* pmf) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_light_pmf_batch: scene was created without a GPU context (no CPU path exists)");
	if (n && (!pos || !light || !pmf)) return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: batch too large");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	NeeLights Lt{};
	if (const int rc = lights_on_device_locked(sc, Lt); rc != PTX_OK) return rc;
	if (Lt.n == 0) return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: the scene's light list is empty");
	if (n == 0) return PTX_OK;
	const bool dev = is_device_ptr(pos);
	if (dev != is_device_ptr(light) || dev != is_device_ptr(pmf))
		return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: pos, light and pmf must all be device or all be host memory");
	if (!dev)
		for (size_t i = 0; i < n; i++)
			if (light[i] < 0 || (uint32_t)light[i] >= Lt.n) return set_err(PTX_ERR_INVALID, "ptx_light_pmf_batch: light " + std::to_string(i) + " is outside the light list");
	Staged s_pos, s_light, s_pmf;   // pos and light share stage_a
	if (!dev) HIP_TRY(c->stage_a.ensure(n * 16));
	HIP_TRY(s_pos.bind(c, dev, pos, n * 12, c->stage_a));
	HIP_TRY(s_light.bind(c, dev, light, n * 4, c->stage_a, n * 12));
	HIP_TRY(s_pmf.bind(c, dev, pmf, n * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(launch_light_pmf(Lt, s_pos.as<float>(), s_light.as<int32_t>(), n, s_pmf.as<float>(), c->stream));
	HIP_TRY(s_pmf.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_material_eval_batch(ptx_scene* sc, const int32_t* surface, const float* uv, size_t n, float* out) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_material_eval_batch: scene is NULL");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_material_eval_batch: scene was created without a GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!surface || !uv || !out) return set_err(PTX_ERR_INVALID, "ptx_material_eval_batch: NULL argument");
	if (n > (size_t)0x7FFFFFFF) return set_err(PTX_ERR_INVALID, "ptx_material_eval_batch: batch too large");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(out);
	if (dev != is_device_ptr(surface) || dev != is_device_ptr(uv))
		return set_err(PTX_ERR_INVALID, "ptx_material_eval_batch: surface, uv and out must all be device or all be host memory");
	Staged s_uv, s_surf, s_out;   // uv and surface share stage_a
	if (!dev) HIP_TRY(c->stage_a.ensure(n * 12));
	HIP_TRY(s_uv.bind(c, dev, uv, n * 8, c->stage_a));
	HIP_TRY(s_surf.bind(c, dev, surface, n * 4, c->stage_a, n * 8));
	HIP_TRY(s_out.bind(c, dev, out, n * 12 * 4, c->stage_b, 0, kOutputOnly));
	HIP_TRY(launch_material_eval(sc->dev, s_surf.as<int32_t>(), s_uv.as<float>(), n, s_out.as<float>(), c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_reduce_framebuffer(ptx_ctx* c, void* nccl_comm, float* accum, size_t n_floats, int root) {
	if (!c || !nccl_comm || !accum) return set_err(PTX_ERR_INVALID, "ptx_reduce_framebuffer: NULL argument");
	if (!is_device_ptr(accum)) return set_err(PTX_ERR_INVALID, "ptx_reduce_framebuffer: accum must be device memory");
	// ncclResult_t ncclReduce(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) — rccl.h
	using reduce_fn = int (*)(const void*, void*, size_t, int, int, int, void*, hipStream_t);
	static reduce_fn fn = [] {
		void* sym = dlsym(RTLD_DEFAULT, "ncclReduce");            // the RCCL that created the communicator, if already loaded
		if (!sym)
			if (void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL)) sym = dlsym(h, "ncclReduce");
		return reinterpret_cast<reduce_fn>(sym);
	}();
	if (!fn) return set_err(PTX_ERR_UNSUPPORTED, "ptx_reduce_framebuffer: no RCCL (ncclReduce) in this process and librccl.so cannot be loaded");
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	constexpr int kNcclFloat32 = 7, kNcclSum = 0;                 // rccl.h: ncclFloat32 = 7, ncclSum = 0
	const int rc = fn(accum, accum, n_floats, kNcclFloat32, kNcclSum, root, nccl_comm, c->stream);
	if (rc != 0) return set_err(PTX_ERR_HIP, "ncclReduce failed with ncclResult_t " + std::to_string(rc));
	return PTX_OK;
}

int ptx_tonemap_encode(ptx_ctx* c, const float* accum, uint32_t W, uint32_t H, uint32_t spp, uint8_t* rgba8) {
	if (!c) return set_err(PTX_ERR_NO_DEVICE, "ptx_tonemap_encode: no GPU context (no CPU path exists)");
	if (!accum || !rgba8 || !W || !H || !spp) return set_err(PTX_ERR_INVALID, "ptx_tonemap_encode: bad argument");
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)W * H;
	const bool dev_in = is_device_ptr(accum), dev_out = is_device_ptr(rgba8);
	Staged s_in, s_out;
	HIP_TRY(s_in.bind(c, dev_in, accum, n * 16, c->stage_a));
	HIP_TRY(s_out.bind(c, dev_out, rgba8, n * 4, c->stage_b, 0, kOutputOnly));
	if (!c->srgb_thr.p) {
		float thr[256];
		srgb_thresholds(thr);
		HIP_TRY(c->srgb_thr.ensure(sizeof thr));
		HIP_TRY(hipMemcpy(c->srgb_thr.p, thr, sizeof thr, hipMemcpyHostToDevice));
	}
	HIP_TRY(launch_tonemap(s_in.as<float4>(), (uint32_t)n, (float)spp, (const float*)c->srgb_thr.p, s_out.as<uchar4>(), c->stream));
	HIP_TRY(s_out.copy_back(c));
	if (!dev_out) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_encode_png(const uint8_t* rgba8, uint32_t W, uint32_t H, uint8_t** png, size_t* png_bytes) {
	if (!rgba8 || !png || !png_bytes || !W || !H) return set_err(PTX_ERR_INVALID, "ptx_encode_png: bad argument");
	const size_t row = (size_t)W * 4;
	std::vector<uint8_t> raw((row + 1) * H);
	for (uint32_t y = 0; y < H; y++) {
		raw[(row + 1) * y] = 0;  // filter type None
		memcpy(&raw[(row + 1) * y + 1], rgba8 + row * y, row);
	}
	uLongf zcap = compressBound((uLong)raw.size());
	std::vector<uint8_t> z(zcap);
	if (compress2(z.data(), &zcap, raw.data(), (uLong)raw.size(), 6) != Z_OK) return set_err(PTX_ERR_INVALID, "zlib compress2 failed");
	const size_t total = 8 + (12 + 13) + (12 + zcap) + 12;
	uint8_t* out = (uint8_t*)malloc(total);
	if (!out) return set_err(PTX_ERR_INVALID, "out of memory");
	uint8_t* p = out;
	static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
	memcpy(p, sig, 8); p += 8;
	auto be32 = [](uint8_t* q, uint32_t v) { q[0] = v >> 24; q[1] = v >> 16; q[2] = v >> 8; q[3] = v; };
	auto chunk = [&](const char* type, const uint8_t* data, uint32_t len) {
		be32(p, len); memcpy(p + 4, type, 4);
		if (len) memcpy(p + 8, data, len);
		be32(p + 8 + len, (uint32_t)crc32(0, p + 4, len + 4));
		p += 12 + len;
	};
	uint8_t ihdr[13];
	be32(ihdr, W); be32(ihdr + 4, H);
	ihdr[8] = 8; ihdr[9] = 6; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;  // 8-bit RGBA
	chunk("IHDR", ihdr, 13);
	chunk("IDAT", z.data(), (uint32_t)zcap);
	chunk("IEND", nullptr, 0);
	*png = out;
	*png_bytes = total;
	return PTX_OK;
}

void ptx_free(void* p) { free(p); }
