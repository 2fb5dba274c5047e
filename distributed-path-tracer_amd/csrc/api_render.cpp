// The render entry points of the C ABI: which pipeline renders a scene, the pixel list, the queue pipeline's plan / pass / stats, and
// ptx_render, ptx_render_transparent, ptx_render_aov, ptx_render_nee, ptx_render_adaptive, ptx_render_adaptive_nee and ptx_intersect_batch.
#include <cmath>

#include "api_internal.hpp"

namespace {

int32_t max_surfaces_per_model(const ptx_scene* sc) {
	int32_t m = 0;
	for (const ModelRec& mr : sc->host.models) m = std::max(m, mr.n_surfaces);
	return m;
}

// Scenes the queue-based pipeline (wavefront.hip) takes: trees in global memory, a model of many surfaces (where the fused kernel's
// waves run nearly empty), at most 64 surfaces (one mask word per ray). PTX_WAVEFRONT=0/1 overrides the choice (measurement).
// Pair space is a pool sized from DEMAND: `wf_pairs_per_ray` of the scene (what its rays were seen to need; before the first
// measurement min(surfaces, 4)) plus a margin decides how many rays a pool of `pool_pairs` serves; a step that needs more raises the
// overflow word and the slab / slice is repeated in smaller pieces with the ratio it reported.
// pairs of a render's pool, 48 B each. Measured on the 24-surface atrium (3.7 pairs per ray, two rays per path and step; 1080p, 64 spp):
// 128 Mi pairs (6 GB: 17 M-path slabs, 10 GB of workspace in all) 409 Msamples/s, 256 Mi 435, 384 Mi 447, 512 Mi 452
// (profiles/round3_wf_ab.txt), and with the queues started largest tree first 384 / 512 Mi 473 / 477, 1024 Mi — the whole 133 M-path
// pass as ONE slab — 490-495 (profiles/round3_surface_order.txt): every step of a slab ends with a few waves finishing walks of
// hundreds of dependent fetches, and a larger slab has fewer such ends per path (jack-of-blades, whose steps after the first are small:
// 2300 -> 2850 Msamples/s from 66 M- to 133 M-path slabs). The default takes 1 Gi pairs (48 GB of a 288 GB device) unless that is more
// than a sixth of the free memory; what is ALLOCATED follows the scene's demand (wf_allocate).
constexpr uint64_t kWfPoolPairs = 1024ull << 20;
constexpr uint64_t kWfBatchPairs = 256ull << 20;   // ... of a batch-intersect slice at most (12 GB); sized by the batch
constexpr uint32_t kWfFlowWords = 64, kWfFlowRays = 58 /* 64-bit */, kWfFlowPeak = 60, kWfFlowOverflow = 63, kWfMaxRound = 56;   // flow words: [s] entries of step s of the round, then the pool's peak demand and the overflow word
// The traverse kernel reads leaf-ordered records at 32-bit offsets from the nodes (k_wf_traverse2), so a scene whose global-memory copy
// holds one record per triangle (PTX_LEAF_ORDER=0, measurement) or takes more than 4 GB goes to the fused kernel: both pipelines give
// bitwise equal results, and no test or benchmark scene reaches either case.
bool wf_eligible(const ptx_scene* sc) {
	const size_t n_surf = sc->host.surfaces.size();
	if (n_surf == 0 || n_surf > (size_t)kWfMaxSurfaces) return false;
	if (sc->mode == MODE_LDS || !sc->dev.tri_isect) return false;   // LDS-resident scenes keep no global-memory copy of the traversal records
	return sc->leaf_ordered && sc->dev.geom_bytes <= 0xFFFFFFFFull;
}
// Which pipeline renders a scene. The fused kernel is at its best when the geometry rays meet is in LDS; the queues, when it is in
// global memory: lanes are compacted per (ray, surface) pair and more waves cover the fetch latency. Two static signs of the latter:
// a model of eight or more surfaces (1.9 x on the 24-surface atrium), or little of the surfaces' box area being LDS-resident — the
// share is 0.98 for Cornell + 82 k-triangle mesh and 0.86 for the plaza (walls / ground resident: the queues run them 0.57 x / 0.73 x),
// 0.16 for the reference's jack-of-blades (1.08 x through the queues) and 0.08 for the atrium. PTX_WAVEFRONT=0/1 overrides
// (measurement, tests); the fused kernel's own measurement switches keep it selected.
int pipeline_choice(const ptx_scene* sc) {
	if (!wf_eligible(sc)) return 0;
	if (const char* e = getenv("PTX_WAVEFRONT")) return e[0] == '1' ? 1 : 0;
	if (getenv("PTX_FORCE_GLOBAL") || getenv("PTX_NO_HYBRID")) return 0;
	return (max_surfaces_per_model(sc) >= 8 || sc->lds_area_share < 0.35) ? 1 : 0;
}
bool use_wavefront(const ptx_scene* sc) { return pipeline_choice(sc) == 1; }
double wf_ratio_guess(const ptx_scene* sc) {
	const double n_surf = (double)sc->host.surfaces.size();
	if (sc->wf_pairs_per_ray > 0) return std::min(n_surf, sc->wf_pairs_per_ray * 1.15 + 0.05);
	if (const char* e = getenv("PTX_WF_RATIO_GUESS")) return std::max(0.01, atof(e));   // tests: a guess that is too low exercises the overflow path
	return std::min(n_surf, 4.0);
}
// buffers of the workspace for `rays` rays per step, a pool of `pool` pairs and `steps` control blocks
hipError_t wf_workspace(ptx_ctx* c, size_t rays, size_t pool, size_t n_surf, size_t steps, WfBuffers& W) {
	ptx_ctx::WfSet& w = c->wf;
	const size_t tiles = (rays + kWfTile - 1) / kWfTile;
	hipError_t e;
	if ((e = w.qent.ensure(pool * 32)) != hipSuccess) return e;
	if ((e = w.pair_hit.ensure(pool * 16)) != hipSuccess) return e;
	if ((e = w.seg.ensure(n_surf * tiles * sizeof(uint2))) != hipSuccess) return e;
	if ((e = w.first.ensure(rays * 4)) != hipSuccess) return e;
	if ((e = w.mask.ensure(rays * 8)) != hipSuccess) return e;
	if ((e = w.ctl.ensure(steps * kWfCtlWords * 4)) != hipSuccess) return e;
	if ((e = w.flow.ensure(kWfFlowWords * 4)) != hipSuccess) return e;
	if (!w.flow_host && (e = hipHostMalloc((void**)&w.flow_host, kWfFlowWords * 4)) != hipSuccess) return e;
	if ((e = w.spill.ensure((size_t)wf_traverse_grid(c->n_cu) * 4 * (size_t)kSpillWords * sizeof(uint4))) != hipSuccess) return e;   // 16-byte entries: node content + entry distance
	W.qent = (float4*)w.qent.p; W.pair_hit = (float4*)w.pair_hit.p;
	W.pool_cap = (uint32_t)std::min<size_t>(pool, 0xFFFFFFFFu);
	W.seg = (uint2*)w.seg.p; W.seg_cap = (uint32_t)tiles;
	W.first = (uint32_t*)w.first.p; W.mask = (unsigned long long*)w.mask.p; W.ctl = (uint32_t*)w.ctl.p; W.spill = (uint2*)w.spill.p;
	W.n_in = nullptr;
	W.overflow = (uint32_t*)w.flow.p + kWfFlowOverflow;
	W.peak = (uint32_t*)w.flow.p + kWfFlowPeak;
	W.ray_counter = nullptr;
	W.wave_clock = 0;
	return hipSuccess;
}
size_t wf_workspace_bytes(const ptx_ctx* c) {
	size_t b = 0;
	const ptx_ctx::WfSet& w = c->wf;
	for (const DevBuf* d : {&w.qent, &w.pair_hit, &w.seg, &w.first, &w.mask, &w.ctl, &w.spill, &w.stream_buf, &w.flow}) b += d->cap;
	return b;
}

// The order in which a pass enumerates its pixels (path id -> pixel). Per-sample radiance is keyed by (pixel, sample), so the order
// changes no result — only which rays sit next to each other in a wave and in a classify tile. "tiled": 8 x 8 pixel blocks (one
// wave of camera rays) inside 32 x 32 blocks (one classify tile) — coherent rays enter the same surfaces and walk the same nodes;
// PTX_PIXEL_ORDER=linear|tiled overrides (measurement). Interleaved tile sharding: only the pixels of this shard's image tiles.
// The list lives on the device, cached on the context by its key. Without sharding or tiling there is none: `d_pixels` stays nullptr
// and `n_pixels` the rectangle's pixels.
int pixel_list(ptx_ctx* c, const ptx_scene* sc, const ptx_render_cfg* cfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint64_t& n_pixels,
               const uint32_t*& d_pixels) {
	const bool sharded = cfg->shard_count > 1;
	bool tiled = use_wavefront(sc);   // measured: profiles/round3_pixel_order.txt
	if (const char* e = getenv("PTX_PIXEL_ORDER")) tiled = e[0] == 't';
	n_pixels = (uint64_t)w * h;
	d_pixels = nullptr;
	if (!sharded && !tiled) return PTX_OK;
	const uint32_t ts = sharded ? (cfg->shard_tile ? cfg->shard_tile : 64u) : 0u;
	const uint32_t key[9] = {cfg->W, cfg->H, x0, y0, w, h, sharded ? cfg->shard_index : 0u, (sharded ? cfg->shard_count : 1u) | (tiled ? 0x80000000u : 0u), ts};
	if (memcmp(key, c->list_key, sizeof key) != 0 || !c->pixel_list.p) {
		std::vector<uint32_t> list;
		// the pixels of the image rectangle [xa, xb) x [ya, yb): rows, or 8 x 8 blocks inside 32 x 32 blocks anchored at the image origin
		auto add_rect = [&](uint32_t xa, uint32_t ya, uint32_t xb, uint32_t yb) {
			if (!tiled) {
				for (uint32_t y = ya; y < yb; y++)
					for (uint32_t x = xa; x < xb; x++) list.push_back((y - y0) * w + (x - x0));
				return;
			}
			for (uint32_t by = ya / 32; by <= (yb - 1) / 32; by++)
				for (uint32_t bx = xa / 32; bx <= (xb - 1) / 32; bx++)
					for (uint32_t sy = 0; sy < 4; sy++)
						for (uint32_t sx = 0; sx < 4; sx++)
							for (uint32_t y = by * 32 + sy * 8; y < by * 32 + sy * 8 + 8; y++)
								for (uint32_t x = bx * 32 + sx * 8; x < bx * 32 + sx * 8 + 8; x++)
									if (x >= xa && x < xb && y >= ya && y < yb) list.push_back((y - y0) * w + (x - x0));
		};
		if (!sharded) add_rect(x0, y0, x0 + w, y0 + h);
		else {
			const uint32_t tiles_x = (cfg->W + ts - 1) / ts;
			for (uint32_t ty = y0 / ts; ty <= (y0 + h - 1) / ts; ty++)
				for (uint32_t tx = x0 / ts; tx <= (x0 + w - 1) / ts; tx++) {
					if ((uint64_t)(ty * (uint64_t)tiles_x + tx) % cfg->shard_count != cfg->shard_index) continue;
					add_rect(std::max(tx * ts, x0), std::max(ty * ts, y0), std::min((tx + 1) * ts, x0 + w), std::min((ty + 1) * ts, y0 + h));
				}
		}
		// a previous render with stats == NULL and a device buffer returns without a sync (ptx.h): its generate / resolve kernels may
		// still be reading the list this call is about to replace, and the context's stream is non-blocking (not ordered with the
		// NULL stream a plain hipMemcpy would use) — drain it first, then upload on the same stream
		HIP_TRY(hipStreamSynchronize(c->stream));
		HIP_TRY(c->pixel_list.ensure(std::max<size_t>(list.size() * 4, 16)));
		if (!list.empty()) {
			HIP_TRY(hipMemcpyAsync(c->pixel_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));   // `list` is a local
		}
		memcpy(c->list_key, key, sizeof key);
		c->list_len = (uint32_t)list.size();
	}
	n_pixels = c->list_len;
	d_pixels = (const uint32_t*)c->pixel_list.p;
	return PTX_OK;
}

// The queue-based pipeline of one render: the pair pool, the slab size and the workspace sized for them
struct WfPlan {
	uint64_t pool_pairs = kWfPoolPairs;   // pair budget
	uint64_t pass_paths = 0;              // paths of a full pass
	uint32_t round = 0;                   // steps enqueued before the host reads the flow words again
	uint32_t slab = 0;                    // paths of a slab: never above what the buffers were sized for
	WfBuffers W{};
};
// ptx_ctx_set_timing on: the step events used so far, and the traverse waves' run times against waves x longest run
struct WfClock {
	size_t n_step_ev = 0;
	double busy = 0, all = 0;
};

// paths of a slab: the pool must hold the pairs of its busiest step — a step classifies two rays per path (extend + shadow)
uint32_t wf_slab_cap(const ptx_scene* sc, const WfPlan& plan) {
	const double per_path = 2.0 * wf_ratio_guess(sc);
	const uint64_t by_pool = (uint64_t)std::max(65536.0, (double)plan.pool_pairs / per_path);
	static const uint64_t max_slab = [] { const char* e = getenv("PTX_WF_MAX_SLAB_M"); return e ? std::min<uint64_t>((uint64_t)kWfIdMask, strtoull(e, nullptr, 10) << 20) : (uint64_t)kWfMaxSlab - 1; }();   // measurement
	const uint64_t cap = std::min<uint64_t>({plan.pass_paths, max_slab, by_pool});
	const uint64_t n_slabs = (plan.pass_paths + cap - 1) / cap;   // slabs of equal size rather than full ones and a remainder
	return (uint32_t)((plan.pass_paths + n_slabs - 1) / n_slabs);
}

// The workspace for slabs of `plan.slab` paths. The pool that is allocated: what the slab needs at the pairs per path this scene is
// expected to ask for (+ 10 %), not the whole budget — a scene whose rays enter few boxes (jack-of-blades: 0.3 pairs per ray) holds
// 2 GB of pairs, not 18 (in steps of 64 Mi pairs: the ratio learnt from one frame must not move the allocation by a few per cent in the next)
hipError_t wf_allocate(ptx_ctx* c, const ptx_scene* sc, WfPlan& plan) {
	const uint64_t want_pairs = (uint64_t)((double)plan.slab * 2.0 * wf_ratio_guess(sc) * 1.1), step = want_pairs > (128ull << 20) ? (64ull << 20) : (16ull << 20);
	const uint64_t alloc_pairs = std::min<uint64_t>(plan.pool_pairs, std::max<uint64_t>(16ull << 20, (want_pairs + step - 1) / step * step));
	ptx_ctx::WfSet& w = c->wf;
	if (w.qent.cap > 4 * alloc_pairs * 32) { w.qent.release(); w.pair_hit.release(); }   // held from a much hungrier scene: give it back
	hipError_t e = wf_workspace(c, 2 * (size_t)plan.slab, alloc_pairs, sc->host.surfaces.size(), plan.round, plan.W);
	if (e != hipSuccess) return e;
	plan.W.ray_counter = (unsigned long long*)((uint32_t*)w.flow.p + kWfFlowRays);   // rays of the slab: added to the total once the slab is through (an overflowing attempt is not counted)
	return w.stream_buf.ensure((size_t)plan.slab * 14 * sizeof(float4));
}

// The plan of a render of passes of `pass_paths` paths. `fits` = false: the device cannot spare even a small pool, the fused kernel renders.
int wf_plan(ptx_ctx* c, const ptx_scene* sc, uint64_t pass_paths, uint32_t bounces, WfPlan& plan, bool& fits) {
	plan.pass_paths = pass_paths;
	// steps enqueued back to back before the host looks at the flow words again. The grids of a round are sized for the entries the
	// slab had when the round began (entries only ever get fewer): short rounds keep the later steps' grids close to what is alive —
	// the shade kernel's workgroups beyond the entry count only read it and leave, but a 66 M-path slab has 259 K of them per launch —
	// at the price of one host round trip (tens of microseconds) per round. PTX_WF_ROUND overrides (measurement).
	uint32_t round = 3;
	if (const char* e = getenv("PTX_WF_ROUND")) round = (uint32_t)std::max(1, atoi(e));
	plan.round = (uint32_t)std::min<uint64_t>({(uint64_t)round, (uint64_t)bounces + 1u, (uint64_t)kWfMaxRound});
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
		const uint64_t held = wf_workspace_bytes(c);   // what the context already holds counts as available: the same answer frame after frame
		plan.pool_pairs = std::min<uint64_t>(plan.pool_pairs, std::max<uint64_t>(16ull << 20, (free_b + held) / 4 / 48));
	} else (void)hipGetLastError();
	if (const char* e = getenv("PTX_WF_PAIRS_M")) plan.pool_pairs = std::max<uint64_t>(1, strtoull(e, nullptr, 10)) << 20;   // measurement: pool size in Mi pairs
	plan.pool_pairs = std::min<uint64_t>(plan.pool_pairs, 0xFFFFFFFFull);
	// when the device cannot spare the pool: a smaller one (smaller slabs), and below 8 Mi pairs the fused kernel
	for (;;) {
		plan.slab = wf_slab_cap(sc, plan);
		const hipError_t e = wf_allocate(c, sc, plan);
		if (e == hipSuccess) { fits = true; return PTX_OK; }
		if (e != hipErrorOutOfMemory) return set_err(PTX_ERR_HIP, std::string("queue-based pipeline workspace: ") + hipGetErrorString(e));
		(void)hipGetLastError();
		ptx_ctx::WfSet& w = c->wf;
		for (DevBuf* b : {&w.qent, &w.pair_hit, &w.seg, &w.first, &w.mask, &w.stream_buf}) b->release();
		plan.pool_pairs /= 2;
		if (plan.pool_pairs < (8ull << 20)) { fits = false; return PTX_OK; }
	}
}

// The scene's first frame has just told what its rays need: bring the workspace to the size the NEXT frame of this kind will ask
// for now (a larger slab, a smaller or larger pool), inside the frame that pays for allocations anyway
int wf_resize(ptx_ctx* c, const ptx_scene* sc, WfPlan& plan) {
	HIP_TRY(hipStreamSynchronize(c->stream));
	plan.slab = wf_slab_cap(sc, plan);
	if (wf_allocate(c, sc, plan) != hipSuccess) (void)hipGetLastError();   // not fatal: the next frame sizes its workspace itself
	return PTX_OK;
}

// four events per step (before classify / traverse / shade, after), or nullptr when timing is off
hipEvent_t* step_events(ptx_ctx* c, WfClock* clk) {
	if (!clk) return nullptr;
	while (c->step_events.size() < clk->n_step_ev + 4) {
		hipEvent_t ev;
		if (hipEventCreate(&ev) != hipSuccess) return nullptr;
		c->step_events.push_back(ev);
	}
	clk->n_step_ev += 4;
	return &c->step_events[clk->n_step_ev - 4];
}

// One pass through the queue-based pipeline (wavefront.hip), in slabs of at most `plan.slab` paths. The steps of a slab are enqueued back
// to back, `plan.round` at a time: every kernel takes its entry count from the device (flow words), and the host reads them back once
// per round — whether paths are left (pass-through materials can outlive bounces + 1 steps), whether some step's pairs overflowed the
// pool, and the peak demand that sizes the next slab. Adds the rays traced (slabs that went through) to `rays`.
int wf_pass(ptx_ctx* c, ptx_scene* sc, const RenderParams& P, float4* sample_rad, bool stats, WfClock* clk, WfPlan& plan, unsigned long long& rays) {
	ptx_ctx::WfSet& ws = c->wf;
	uint32_t* const flow = (uint32_t*)ws.flow.p;
	uint64_t first = 0;
	while (first < P.n_paths) {
		plan.slab = std::min(plan.slab, wf_slab_cap(sc, plan));
		const uint32_t cap = plan.slab;
		float4* const base = (float4*)ws.stream_buf.p;   // the slab's two stream buffers, `cap` entries per array
		const WfStream st[2] = {WfStream{base, base + 8 * (size_t)cap}, WfStream{base + 4 * (size_t)cap, base + 11 * (size_t)cap}};
		const uint32_t slab_first = (uint32_t)first, n_slab = (uint32_t)std::min<uint64_t>(cap, P.n_paths - first);
		HIP_TRY(launch_wf_generate(sc->dev, P, st[0], cap, slab_first, n_slab, sample_rad, c->stream));
		HIP_TRY(hipMemsetAsync(ws.flow.p, 0, kWfFlowWords * 4, c->stream));
		HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ws.flow.p, (int)n_slab, 1, c->stream));   // flow[0] = entries of step 0
		bool live = P.bounces > 0, overflow = false;
		uint32_t n_round = n_slab;   // entries when the current round began
		int cur = 0;
		uint64_t peak = 0;
		while (live) {
			HIP_TRY(hipMemsetAsync(ws.ctl.p, 0, (size_t)plan.round * kWfCtlWords * 4, c->stream));
			HIP_TRY(hipMemsetAsync(flow + 1, 0, (size_t)plan.round * 4, c->stream));
			for (uint32_t s = 0; s < plan.round; s++) {
				WfBuffers W = plan.W;
				W.ctl = (uint32_t*)ws.ctl.p + (size_t)s * kWfCtlWords;
				W.n_in = flow + s;
				W.wave_clock = clk ? 1u : 0u;
				HIP_TRY(launch_wf_step(sc->dev, P, W, st[cur], st[cur ^ 1], cap, n_round, slab_first, flow + s + 1, sample_rad, c->n_cu, c->stream, step_events(c, clk)));
				cur ^= 1;
			}
			HIP_TRY(hipMemcpyAsync(ws.flow_host, flow, kWfFlowWords * 4, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			peak = std::max<uint64_t>(peak, ws.flow_host[kWfFlowPeak]);
			if (clk) {   // the traverse waves' own clocks of this round's steps (wavefront.hip: kWfCtlClock)
				for (uint32_t s = 0; s < plan.round; s++) {
					uint32_t ck[4];
					HIP_TRY(hipMemcpy(ck, (uint32_t*)ws.ctl.p + (size_t)s * kWfCtlWords + kWfCtlClock, sizeof ck, hipMemcpyDeviceToHost));
					clk->busy += (double)(((uint64_t)ck[1] << 32) | ck[0]);
					clk->all += (double)ck[2] * (double)ck[3];
				}
			}
			if (ws.flow_host[kWfFlowOverflow]) { overflow = true; break; }
			n_round = ws.flow_host[plan.round];
			live = n_round != 0;
			if (live) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ws.flow.p, (int)n_round, 1, c->stream));   // next round: flow[0] = what this one left
		}
		// what a ray of this scene needs, from the busiest step of the slab (two rays per path and step)
		if (peak && n_slab) sc->wf_pairs_per_ray = std::max(sc->wf_pairs_per_ray, (double)peak / (2.0 * n_slab));
		if (stats) { c->timing.peak_pairs = std::max<uint64_t>(c->timing.peak_pairs, peak); c->timing.slab_paths = std::max<uint64_t>(c->timing.slab_paths, n_slab); }
		if (overflow) {
			if (stats) c->timing.pool_overflows++;
			// some step needed more pairs than the pool holds: the same slab again, smaller (the ratio just learnt says how much). The
			// samples the aborted attempt already stored are stored again with the same values.
			HIP_TRY(hipStreamSynchronize(c->stream));
			const uint32_t smaller = std::min<uint32_t>(wf_slab_cap(sc, plan), cap - cap / 4);
			if (cap <= 4096) return set_err(PTX_ERR_HIP, "queue-based pipeline: the pair pool cannot hold one step of a 4096-path slab");
			plan.slab = std::max<uint32_t>(4096, smaller);
			continue;
		}
		if (n_slab && P.bounces > 0) { unsigned long long r; memcpy(&r, ws.flow_host + kWfFlowRays, 8); rays += r; }
		first += cap;
	}
	return PTX_OK;
}

// ptx_render_stats of a finished render, and the context's ptx_kernel_timing (PTX_CLK / PTX_PROF builds: region clocks and counters
// of the fused kernel on stderr)
int render_stats(ptx_ctx* c, const PassFrame& f, bool wavefront, const WfPlan& plan, const WfClock& clk, unsigned long long wf_rays, ptx_render_stats* stats) {
	unsigned long long rays = 0;
	HIP_TRY(hipMemcpy(&rays, (char*)c->counters.p + 16, 8, hipMemcpyDeviceToHost));
	if (const int rc = f.stats(c, rays + wf_rays, stats); rc != PTX_OK) return rc;
	const double ms = stats->kernel_ms;
	ptx_kernel_timing& tm = c->timing;
	tm.pipeline = wavefront ? 1u : 0u;
	tm.pool_pairs = wavefront ? plan.W.pool_cap : 0;
	tm.workspace_bytes = wavefront ? wf_workspace_bytes(c) : c->queues.cap + c->spill.cap;
	if (!wavefront) { tm.fused_ms = ms; tm.fused_launches = f.n_pass; }
	for (size_t k = 0; k + 4 <= clk.n_step_ev; k += 4) {
		float t0 = 0, t1 = 0, t2 = 0;
		HIP_TRY(hipEventElapsedTime(&t0, c->step_events[k], c->step_events[k + 1]));
		HIP_TRY(hipEventElapsedTime(&t1, c->step_events[k + 1], c->step_events[k + 2]));
		HIP_TRY(hipEventElapsedTime(&t2, c->step_events[k + 2], c->step_events[k + 3]));
		tm.classify_ms += t0; tm.traverse_ms += t1; tm.shade_ms += t2;
		tm.steps++;
	}
	tm.traverse_drain_frac = clk.all > 0 ? 1.0 - clk.busy / clk.all : 0.0;
#ifdef PTX_CLK
	if (!wavefront) {
		unsigned long long clks[8];
		HIP_TRY(hipMemcpy(clks, (char*)c->counters.p + 64, sizeof clks, hipMemcpyDeviceToHost));
		static const char* names[8] = {"kernel", "chunk_fetch", "extend_entry_loads", "extend_sweep_rest", "set_aside_lists", "shade_entry_hit_loads", "shade_hitrec_gathers", "shade_rest"};
		for (int k = 0; k < 8; k++) fprintf(stderr, "CLK %-22s %12llu kcycles summed over waves (%.2f %% of the waves' time)\n", names[k], clks[k], 100.0 * clks[k] / (double)clks[0]);
	}
#endif
#ifdef PTX_PROF
	unsigned long long prof[2 * kProfRegions];
	HIP_TRY(hipMemcpy(prof, (char*)c->counters.p + 64, sizeof prof, hipMemcpyDeviceToHost));
	static const char* names[kProfRegions] = {"extend_iter", "model_iter", "space_xform", "inline_model", "mesh_call", "mesh_pop", "node_step",
	                                           "tri_test", "defer_iter", "shade_iter", "defer_mesh_call", "defer_mesh_pop", "defer_node_step", "defer_tri_test",
	                                           "list_append", "shade_hit", "vertex_miss", "vertex_back_face", "vertex_last", "vertex_full",
	                                           "leaf_only_call", "complete_pop", "complete_node_step", "defer_leaf_only_call", "defer_complete_pop", "defer_complete_node_step",
	                                           "chain_level", "defer_chain_level"};
	for (int k = 0; k < kProfRegions; k++)
		fprintf(stderr, "PROF %-16s trips %12llu lanes %14llu  util %.3f  trips/64rays %.3f\n", names[k], prof[2 * k], prof[2 * k + 1],
		        prof[2 * k] ? (double)prof[2 * k + 1] / (64.0 * prof[2 * k]) : 0.0, (double)prof[2 * k] / ((double)rays / 64.0));
#endif
	return PTX_OK;
}

// The caller holds the context's mutex and has set its device. `who`: the entry point, for the messages.
int render_frame_locked(ptx_scene* sc, const ptx_render_cfg* cfg, const char* who, float* accum, uint8_t* claimed, ptx_render_stats* stats, const PixelSubset* subset) {
	PassFrame f;
	f.cfg = cfg;
	if (const int rc = render_rect(cfg, who, true, f.x0, f.y0, f.w, f.h); rc != PTX_OK) return rc;
	ptx_ctx* c = sc->ctx;
	if (stats) *stats = ptx_render_stats{};
	// by default 128 Mi paths per pass — 64 spp of a 1080p frame: 2 GB of per-sample radiance; fewer, longer launches (measured: 8 -> 64 spp
	// per launch = +11 %); path ids are 32-bit
	if (const int rc = f.plan(c, sc, who, subset, 128ull << 20, 0xFFFFFFFFull); rc != PTX_OK || !f.n_pass) return rc;
	const uint32_t pass_spp = f.pass_spp, n_pass = f.n_pass;
	const uint64_t n_pixels = f.n_pixels;

	const int grid = c->n_cu;
	const size_t n_slots = (size_t)grid * (kBlock / 64);
	// Units the fused kernel may set aside: whole models, or — when some model has many surfaces (a Sponza-class mesh) — single
	// surfaces. PTX_SURFACE_UNITS=0/1 overrides the choice (measurement).
	const uint32_t n_surf = (uint32_t)sc->host.surfaces.size(), n_mod = (uint32_t)sc->host.models.size();
	bool surface_units = max_surfaces_per_model(sc) >= 8 && n_surf <= (uint32_t)kMaxDeferModels;   // measured: +49 % on a 24-surface model, -2..-7 % on scenes of 1-3 surfaces per model
	if (const char* e = getenv("PTX_SURFACE_UNITS")) surface_units = e[0] == '1' && n_surf <= (uint32_t)kMaxDeferModels;
	const uint32_t queue_stride = queue_float4_per_wave(surface_units ? n_surf : n_mod);
	bool wavefront = use_wavefront(sc);
	HIP_TRY(c->sample_rad.ensure((size_t)pass_spp * n_pixels * sizeof(float4)));
	HIP_TRY(c->counters.ensure(1024));   // [0] chunk counter, [16] ray counter, [64..] PTX_PROF region counters
	HIP_TRY(c->spill.ensure(n_slots * (size_t)kSpillWords * sizeof(uint2)));
	unsigned long long* chunk_counter = (unsigned long long*)c->counters.p;
	unsigned long long* ray_counter = (unsigned long long*)((char*)c->counters.p + 16);
	HIP_TRY(hipMemsetAsync(c->counters.p, 0, 1024, c->stream));

	const bool dev_accum = is_device_ptr(accum);
	Staged s_accum, s_claimed;
	HIP_TRY(s_accum.bind(c, dev_accum, accum, f.rect_pixels() * sizeof(float4), c->stage_a));
	if (claimed) HIP_TRY(s_claimed.bind(c, dev_accum, claimed, f.rect_pixels(), c->stage_b));
	float4* const d_accum = s_accum.as<float4>();
	uint8_t* const d_claimed = s_claimed.as<uint8_t>();

	if (stats)
		if (const int rc = PassFrame::ensure_events(c, n_pass); rc != PTX_OK) return rc;
	PassBuffers B{nullptr /* the fused kernel's streams: set below, once it is known which pipeline runs */, queue_stride, surface_units ? 1u : 0u, (float4*)c->sample_rad.p, (uint2*)c->spill.p, chunk_counter, ray_counter};
	WfPlan plan;
	WfClock clk;
	unsigned long long wf_rays = 0;   // rays the queue-based pipeline traced (slabs that went through)
	const double ratio_at_entry = sc->wf_pairs_per_ray;
	const bool timing = stats && c->timing_on;
	if (stats) c->timing = ptx_kernel_timing{};
	if (wavefront)   // a device that cannot spare a pool sets `wavefront` to false: the fused kernel renders
		if (const int rc = wf_plan(c, sc, (uint64_t)pass_spp * n_pixels, cfg->bounces, plan, wavefront); rc != PTX_OK) return rc;
	if (!wavefront) {
		HIP_TRY(c->queues.ensure(n_slots * (size_t)queue_stride * sizeof(float4)));
		B.queues = (float4*)c->queues.p;
	}
	for (uint32_t p = 0; p < n_pass; p++) {
		RenderParams P = f.params(p, true);
		P.transparent = claimed ? 1u : 0u;
		HIP_TRY(hipMemsetAsync(chunk_counter, 0, 8, c->stream));
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		if (wavefront) {
			if (const int rc = wf_pass(c, sc, P, B.sample_rad, stats != nullptr, timing ? &clk : nullptr, plan, wf_rays); rc != PTX_OK) return rc;
			if (ratio_at_entry == 0 && sc->wf_pairs_per_ray > 0 && p + 1 == n_pass)
				if (const int rc = wf_resize(c, sc, plan); rc != PTX_OK) return rc;
		} else {
			if (!B.queues || !B.sample_rad || !B.spill) return set_err(PTX_ERR_HIP, "ptx_render: workspace of the fused kernel is not allocated");
			HIP_TRY(launch_render_pass(sc->dev, P, B, sc->mode, sc->lds_bytes, grid, c->stream));
		}
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		if (claimed) HIP_TRY(launch_resolve_claim(B.sample_rad, d_accum, d_claimed, f.d_pixels, P.n_pixels, P.pass_spp, P.sample0, c->stream));
		else HIP_TRY(launch_resolve(B.sample_rad, d_accum, f.d_pixels, P.n_pixels, P.pass_spp, c->stream));
	}
	HIP_TRY(s_accum.copy_back(c));
	HIP_TRY(s_claimed.copy_back(c));
	if (stats || !dev_accum) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) return render_stats(c, f, wavefront, plan, clk, wf_rays, stats);
	return PTX_OK;
}

// ptx_render (claimed == nullptr: `accum` receives sums) and ptx_render_transparent (`accum` and `claimed` are the reference's per-pixel
// blend state, advanced through the samples in order) — the same passes, a different resolve kernel behind each
int render_frame(ptx_scene* sc, const ptx_render_cfg* cfg, const char* who, float* accum, uint8_t* claimed, ptx_render_stats* stats) {
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	return render_frame_locked(sc, cfg, who, accum, claimed, stats, nullptr);
}

}  // namespace

// after render_rect: the pixels and the pass size
int PassFrame::plan(ptx_ctx* c, const ptx_scene* sc, const char* who, const PixelSubset* subset, uint64_t default_samples, uint64_t max_ids) {
	n_pass = 0;
	if (cfg->spp == 0) return PTX_OK;
	if (subset) {
		n_pixels = subset->n_pixels;
		d_pixels = subset->d_pixels;
	} else if (const int rc = pixel_list(c, sc, cfg, x0, y0, w, h, n_pixels, d_pixels); rc != PTX_OK) return rc;
	if (n_pixels == 0) return PTX_OK;   // no tile of this shard meets the rectangle
	pass_spp = pass_size(cfg, n_pixels, default_samples, max_ids);
	if (pass_spp == 0) return set_err(PTX_ERR_INVALID, std::string(who) + ": tile too large for one pass");
	n_pass = (cfg->spp + pass_spp - 1) / pass_spp;
	return PTX_OK;
}

int ptx_render(ptx_scene* sc, const ptx_render_cfg* cfg, float* accum, ptx_render_stats* stats) {
	if (!sc || !cfg || !accum) return set_err(PTX_ERR_INVALID, "ptx_render: NULL argument");
	if (motion_active(sc)) return refuse_motion("ptx_render");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render: scene was created without a GPU context (no CPU path exists)");
	return render_frame(sc, cfg, "ptx_render", accum, nullptr, stats);
}

int ptx_render_transparent(ptx_scene* sc, const ptx_render_cfg* cfg, float* pixel_rgba, uint8_t* claimed, ptx_render_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !pixel_rgba || !claimed) return set_err(PTX_ERR_INVALID, "ptx_render_transparent: NULL argument");
	if (motion_active(sc)) return refuse_motion("ptx_render_transparent");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_transparent: PTX_INTEGRATOR_WORKER has no transparent-background mode here (the worker takes the alpha of the "
		                                    "path's last vertex and jitters sample 0 in this mode, and nothing pins that); use PTX_INTEGRATOR_LIB");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_transparent: scene was created without a GPU context (no CPU path exists)");
	if (is_device_ptr(pixel_rgba) != is_device_ptr(claimed)) return set_err(PTX_ERR_INVALID, "ptx_render_transparent: pixel_rgba and claimed must both be device or both be host memory");
	return render_frame(sc, cfg, "ptx_render_transparent", pixel_rgba, claimed, stats);
}

namespace {

// The scene's motion as the unfused integrators' kernels take it; all zero (active == 0) without active motion. The caller holds the
// context's mutex.
RenderMotion render_motion(const ptx_scene* sc) {
	RenderMotion R{};
	const FlatScene::Motion& mo = sc->host.motion;
	if (!mo.active()) return R;
	R.active = 1u;
	R.camera_moved = mo.camera_moved ? 1u : 0u;
	R.models_moved = mo.any_model() ? 1u : 0u;
	if (R.models_moved) R.models = sc->dev_motion;
	memcpy(R.cam_begin, mo.begin_camera, sizeof R.cam_begin);
	R.shutter_open = mo.shutter_open;
	R.shutter_close = mo.shutter_close;
	return R;
}

// Closest hits of the A.n rays of `A` (device memory) on the scene's own route — the routing body of ptx_intersect_batch, shared with
// ptx_render_aov: the queue-based pipeline in slices with its overflow / retry handling, or the fused kernel's traversal. The caller holds
// the context's mutex and has set the device. With A.time set (and A.motion with it) every ray has a time: the motion kernels of either route.
int intersect_device(ptx_ctx* c, ptx_scene* sc, IntersectArgs& A) {
	if (use_wavefront(sc)) {
		// queue-based pipeline, a slice of the batch at a time: as many rays as the pool serves at the pairs per ray this scene was seen
		// to need; a slice whose pairs do not fit is repeated smaller (the ratio it reported is remembered on the scene)
		const size_t n = A.n;
		const size_t n_surf = sc->host.surfaces.size();
		// the pool: what the whole batch is expected to need (in steps of 16 Mi pairs), at most kWfBatchPairs — one launch for a batch of
		// up to ~60 M rays of a 24-surface scene; larger batches go in slices
		uint64_t pool_pairs = std::min<uint64_t>(kWfBatchPairs, (((uint64_t)((double)n * wf_ratio_guess(sc) * 1.1) >> 24) + 1) << 24);
		if (const char* e = getenv("PTX_WF_PAIRS_M")) pool_pairs = std::max<uint64_t>(1, strtoull(e, nullptr, 10)) << 20;
		auto slice_cap = [&]() { return (size_t)std::max(16384.0, (double)pool_pairs / wf_ratio_guess(sc)); };
		size_t slice = std::min<size_t>(n, slice_cap());
		WfBuffers W{};
		HIP_TRY(wf_workspace(c, slice, pool_pairs, n_surf, 1, W));
		ptx_ctx::WfSet& ws = c->wf;
		for (size_t first = 0; first < n;) {
			const uint32_t m = (uint32_t)std::min(slice, n - first);
			HIP_TRY(hipMemsetAsync(ws.ctl.p, 0, kWfCtlWords * 4, c->stream));
			HIP_TRY(hipMemsetAsync(ws.flow.p, 0, kWfFlowWords * 4, c->stream));
			DevScene batch_dev = sc->dev;
			batch_dev.wf_order += sc->dev.n_surfaces;   // the batch order of the queues (upload_scene)
			HIP_TRY(launch_wf_intersect(batch_dev, A, first, m, W, c->n_cu, c->stream));
			HIP_TRY(hipMemcpyAsync(ws.flow_host, ws.flow.p, kWfFlowWords * 4, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			if (ws.flow_host[kWfFlowPeak]) sc->wf_pairs_per_ray = std::max(sc->wf_pairs_per_ray, (double)ws.flow_host[kWfFlowPeak] / (double)m);
#ifdef PTX_WF_PROF
			uint32_t ctl[kWfCtlCur];
			HIP_TRY(hipMemcpy(ctl, W.ctl, sizeof ctl, hipMemcpyDeviceToHost));
			const uint32_t* pr = ctl + kWfCtlProf;
			static const char* names[8] = {"outer_round", "busy_round", "node_step", "tri_test", "hand_out", "unit_fetch", "pop", "stack_spill"};
			fprintf(stderr, "WFPROF rays %u pairs %u (%.2f per ray)\n", m, ctl[0], (double)ctl[0] / (double)m);
			for (int k = 0; k < 8; k++)
				fprintf(stderr, "WFPROF %-12s trips %10u lanes %11u  util %.3f  lanes/pair %.2f\n", names[k], pr[2 * k], pr[2 * k + 1],
				        pr[2 * k] ? (double)pr[2 * k + 1] / (64.0 * pr[2 * k]) : 0.0, (double)pr[2 * k + 1] / (double)ctl[0]);
			static const char* tn[6] = {"kernel", "unit_fetch", "hand_out", "pop", "descend", "leaf"};
			fprintf(stderr, "WFHIST waves by log2(kilocycles of their run):");
			for (int k = 0; k < 31; k++) if (pr[32 + k]) fprintf(stderr, " [2^%d]=%u", k, pr[32 + k]);
			fprintf(stderr, "  waves that never had a busy round: %u\n", pr[32 + 31]);
			fprintf(stderr, "WFMAX slowest wave %u kcycles, most trips of a wave %u, longest walk of a lane %u steps\n", pr[24], pr[25], pr[26]);
			for (int k = 0; k < 6; k++) fprintf(stderr, "WFCLK %-10s %10u kcycles summed over waves (%.1f %%)\n", tn[k], pr[16 + k], 100.0 * pr[16 + k] / (double)pr[16]);
#endif
			if (ws.flow_host[kWfFlowOverflow]) {
				c->timing.pool_overflows++;
				if (slice <= 16384) return set_err(PTX_ERR_HIP, "queue-based pipeline: the pair pool cannot hold a 16384-ray slice");
				slice = std::max<size_t>(16384, std::min(slice_cap(), slice - slice / 4));
				continue;   // the same rays again, fewer at a time
			}
			first += m;
		}
	} else {
		const int grid = (int)std::min<size_t>((size_t)c->n_cu, (A.n + kBlock - 1) / kBlock);
		HIP_TRY(c->spill.ensure((size_t)c->n_cu * (kBlock / 64) * (size_t)kSpillWords * sizeof(uint2)));
		A.spill = (uint2*)c->spill.p;
		if (A.time) HIP_TRY(launch_intersect_motion(sc->dev, A, sc->mode, sc->lds_bytes, grid, c->stream));
		else HIP_TRY(launch_intersect(sc->dev, A, sc->mode, sc->lds_bytes, grid, c->stream));
	}
	return PTX_OK;
}

}  // namespace

namespace {

// ptx_intersect_batch (time == nullptr) and ptx_intersect_batch_motion: the same refusals and staging. A time array is used only while
// the scene's motion is active; without it the call is ptx_intersect_batch, launch for launch.
int intersect_batch(const char* who_c, ptx_scene* sc, const ptx_rays* r, const float* time, size_t n, const ptx_hits* hh) {
	const std::string who = who_c;
	if (!sc || !r || !hh) return set_err(PTX_ERR_INVALID, who + ": NULL argument");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, who + ": scene was created without a GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!r->ox || !r->oy || !r->oz || !r->dx || !r->dy || !r->dz || !hh->distance || !hh->surface || !hh->triangle || !hh->b0 || !hh->b1 || !hh->b2)
		return set_err(PTX_ERR_INVALID, who + ": required array is NULL");
	auto group_ok = [](const void* a, const void* b, const void* c) { return (!a && !b && !c) || (a && b && c); };
	if (!group_ok(hh->px, hh->py, hh->pz) || !group_ok(hh->nx, hh->ny, hh->nz) || ((hh->u != nullptr) != (hh->v != nullptr)))
		return set_err(PTX_ERR_INVALID, who + ": optional outputs must be given as whole groups");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(r->ox);
	// the time of a ray matters only where a model moves: a moving camera alone leaves every ray's scene the scene at u = 1
	const bool timed = time && sc->host.motion.set && sc->host.motion.any_model();
	if (timed && is_device_ptr(time) != dev) return set_err(PTX_ERR_INVALID, who + ": time must be device or host memory as the rays are");
	IntersectArgs A{};
	A.n = n;
	const int n_out = 6 + (hh->px ? 3 : 0) + (hh->nx ? 3 : 0) + (hh->u ? 2 : 0);
	// host arrays are staged one by one: the rays (and their times) in stage_a, the outputs that were asked for in stage_b, each group `n` entries apart
	if (!dev) {
		HIP_TRY(c->stage_a.ensure((timed ? 7 : 6) * n * 4));
		HIP_TRY(c->stage_b.ensure((size_t)n_out * n * 4));
	}
	const float* const src[6] = {r->ox, r->oy, r->oz, r->dx, r->dy, r->dz};
	void* const dst[14] = {hh->distance, hh->surface, hh->triangle, hh->b0, hh->b1, hh->b2, hh->px, hh->py, hh->pz, hh->nx, hh->ny, hh->nz, hh->u, hh->v};
	Staged in[6], o[14], s_time;
	for (int k = 0; k < 6; k++) HIP_TRY(in[k].bind(c, dev, src[k], n * 4, c->stage_a, k * n * 4));
	if (timed) {
		HIP_TRY(s_time.bind(c, dev, time, n * 4, c->stage_a, 6 * n * 4));
		A.time = s_time.as<float>();
		A.motion = sc->dev_motion;
	}
	for (size_t k = 0, slot = 0; k < 14; k++)
		if (dst[k]) HIP_TRY(o[k].bind(c, dev, dst[k], n * 4, c->stage_b, slot++ * n * 4, kOutputOnly));
	A.ox = in[0].as<float>(); A.oy = in[1].as<float>(); A.oz = in[2].as<float>(); A.dx = in[3].as<float>(); A.dy = in[4].as<float>(); A.dz = in[5].as<float>();
	A.distance = o[0].as<float>(); A.surface = o[1].as<int32_t>(); A.triangle = o[2].as<int32_t>();
	A.b0 = o[3].as<float>(); A.b1 = o[4].as<float>(); A.b2 = o[5].as<float>();
	A.px = o[6].as<float>(); A.py = o[7].as<float>(); A.pz = o[8].as<float>(); A.nx = o[9].as<float>(); A.ny = o[10].as<float>(); A.nz = o[11].as<float>();
	A.u = o[12].as<float>(); A.v = o[13].as<float>();
	if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
	for (const Staged& s : o) HIP_TRY(s.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

}  // namespace

int ptx_intersect_batch(ptx_scene* sc, const ptx_rays* r, size_t n, const ptx_hits* hh) { return intersect_batch("ptx_intersect_batch", sc, r, nullptr, n, hh); }

int ptx_intersect_batch_motion(ptx_scene* sc, const ptx_rays* r, const float* time, size_t n, const ptx_hits* hh) {
	if (!time && n) return set_err(PTX_ERR_INVALID, "ptx_intersect_batch_motion: time is NULL");
	return intersect_batch("ptx_intersect_batch_motion", sc, r, time, n, hh);
}

namespace {

// ptx_render_aov, ptx_render_motion and ptx_render_emission: the same refusals about the cfg and the scene, the same passes and rounds.
// AovKind::guides: the two guide buffers (either may be NULL); else `albedo_cov` is the motion or the emission buffer and the shade kernel
// writes one record per sample. `prev` (motion alone; checked by the caller; may be NULL) is the previous frame.
enum class AovKind { guides, motion, emission };
int aov_frame(ptx_scene* sc, const ptx_render_cfg* cfg, const char* who_c, float* albedo_cov, float* normal_depth, AovKind kind, const ptx_motion_prev* prev,
              ptx_render_stats* stats) {
	const bool motion = kind == AovKind::motion;
	const std::string who = who_c;
	if (kind != AovKind::guides && motion_active(sc)) return refuse_motion(who_c);   // the guide buffers know the shutter; motion vectors and emission do not
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, who + ": PTX_INTEGRATOR_WORKER has no first-hit buffers here (the worker's opacity handling and its un-jittered "
		                                    "sample 0 are not pinned); use PTX_INTEGRATOR_LIB");
	if (cfg->integrator > PTX_INTEGRATOR_WORKER) return set_err(PTX_ERR_INVALID, who + ": unknown integrator");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, who + ": scene was created without a GPU context (no CPU path exists)");
	PassFrame f;
	f.cfg = cfg;
	if (const int rc = render_rect(cfg, who_c, false /* bounces are ignored */, f.x0, f.y0, f.w, f.h); rc != PTX_OK) return rc;
	const bool dev_out = is_device_ptr(albedo_cov ? albedo_cov : normal_depth);
	if (albedo_cov && normal_depth && is_device_ptr(normal_depth) != dev_out)
		return set_err(PTX_ERR_INVALID, who + ": albedo_cov and normal_depth must both be device or both be host memory");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_render_stats{};
	// The workspace holds two ray streams, the hits and two records per sample (120 B), so the default bounds a pass by samples, not by the
	// frame: 32 Mi (16 spp of a 1080p frame, 3.8 GB); sample ids are 32-bit
	if (const int rc = f.plan(c, sc, who_c, nullptr, 32ull << 20, 0xFFFFFFFFull); rc != PTX_OK || !f.n_pass) return rc;

	// workspace of one pass of `cap` samples: [256 B: live counts][stream 0][stream 1][hits][records: two per sample, one for
	// ptx_render_motion and ptx_render_emission], then the previous transforms and the moved words of ptx_render_motion
	const size_t cap = ((size_t)f.pass_spp * f.n_pixels + 3) & ~(size_t)3;   // array stride: keeps the float4 records 16-byte aligned
	// the previous frame, read under the mutex the setters take: the camera (the scene's own when it did not move) and which models moved
	const FlatScene& h = sc->host;
	AovMotion Mo{};
	std::vector<uint32_t> moved;
	const float* prev_xform = nullptr;
	if (motion) {
		memcpy(Mo.origin, h.camera.origin, 12);
		memcpy(Mo.basis, h.camera.basis, 36);
		Mo.tan_half_fov = h.camera.tan_half_fov;
		if (prev && prev->camera) {
			memcpy(Mo.origin, prev->camera->origin, 12);
			memcpy(Mo.basis, prev->camera->basis, 36);
			Mo.tan_half_fov = std::tan(prev->camera->yfov * 0.5F);   // as ptx_scene_set_camera computes it
		}
		if (prev && prev->model_xform) {
			moved.resize(prev->n_models);
			for (size_t m = 0; m < moved.size(); m++) {
				moved[m] = memcmp(prev->model_xform + 12 * m, &h.model_xform[12 * m], 48) != 0;
				if (moved[m]) prev_xform = prev->model_xform;
			}
		}
	}
	const size_t n_models = prev_xform ? moved.size() : 0;
	const RenderMotion Rm = render_motion(sc);   // active only for the guides (the other kinds were refused above)
	uint32_t* live_count = nullptr;
	AovStream st[2];
	float* hits = nullptr;
	float4* rec = nullptr;
	float* times = nullptr;   // under motion of a model: the time of each ray of the round, in stream order
	float* d_xform = nullptr;
	uint32_t* d_moved = nullptr;
	auto carve = [&](void* base) {
		Carver k(base);
		live_count = k.take<uint32_t>(64);
		for (AovStream& s : st) {
			s.ox = k.take<float>(cap); s.oy = k.take<float>(cap); s.oz = k.take<float>(cap);
			s.dx = k.take<float>(cap); s.dy = k.take<float>(cap); s.dz = k.take<float>(cap);
			s.id = k.take<uint32_t>(cap); s.pass = k.take<uint32_t>(cap);
		}
		hits = k.take<float>(6 * cap);
		rec = k.take<float4>((kind == AovKind::guides ? 2 : 1) * cap);
		d_xform = k.take<float>(12 * n_models);
		d_moved = k.take<uint32_t>(n_models);
		times = k.take<float>(Rm.models_moved ? cap : 0);
		return k.off;
	};
	HIP_TRY(c->round_ws.ensure(carve(nullptr)));
	carve(c->round_ws.p);
	if (prev_xform) {   // behind whatever still reads the workspace; the sources are the caller's array and a local: synchronised before they go
		HIP_TRY(hipMemcpyAsync(d_xform, prev_xform, 48 * n_models, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_moved, moved.data(), 4 * n_models, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		Mo.prev_xform = d_xform;
		Mo.moved = d_moved;
	}

	Staged s_albedo, s_normal;
	if (albedo_cov) HIP_TRY(s_albedo.bind(c, dev_out, albedo_cov, f.rect_pixels() * sizeof(float4), c->stage_a));
	if (normal_depth) HIP_TRY(s_normal.bind(c, dev_out, normal_depth, f.rect_pixels() * sizeof(float4), c->stage_b));

	if (stats)
		if (const int rc = PassFrame::ensure_events(c, f.n_pass); rc != PTX_OK) return rc;
	const bool follow = sc->dev.any_alpha != 0;   // some material can pass a sample through: the live count decides when a pass is over
	uint64_t rays = 0;
	for (uint32_t p = 0; p < f.n_pass; p++) {
		RenderParams P = f.params(p, false);
		P.integrator = PTX_INTEGRATOR_LIB;
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		HIP_TRY(launch_aov_generate(sc->dev, P, st[0], (uint32_t)P.n_paths, Rm, c->stream));
		uint32_t live = (uint32_t)P.n_paths;
		for (uint32_t round = 0; live != 0; round++) {
			AovStream in = st[round & 1u];
			if (round == 0) { in.id = nullptr; in.pass = nullptr; }   // entry i is sample i
			IntersectArgs A{};
			A.n = live;
			ray_args(A, in.ox, cap);
			hit_args(A, hits, cap);
			if (Rm.models_moved) {   // a time per ray: the sample's, whichever round its ray is in
				HIP_TRY(launch_motion_times(P, Rm, in.id, live, times, c->stream));
				A.time = times;
				A.motion = Rm.models;
			}
			if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
			rays += live;
			const AovHits H{A.surface, A.triangle, A.b1, A.b2};
			uint32_t* const n_out = live_count + (round & 1u);
			if (follow) HIP_TRY(hipMemsetAsync(n_out, 0, 4, c->stream));
			if (motion) HIP_TRY(launch_aov_motion_shade(sc->dev, P, in, H, live, st[(round + 1u) & 1u], n_out, rec, Mo, c->stream));
			else if (kind == AovKind::emission) HIP_TRY(launch_aov_emission_shade(sc->dev, P, in, H, live, st[(round + 1u) & 1u], n_out, rec, c->stream));
			else HIP_TRY(launch_aov_shade(sc->dev, P, in, H, live, st[(round + 1u) & 1u], n_out, rec, cap, Rm, c->stream));
			if (!follow) break;
			HIP_TRY(hipMemcpyAsync(&live, n_out, 4, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
		}
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		HIP_TRY(launch_aov_resolve(rec, cap, s_albedo.as<float4>(), s_normal.as<float4>(), f.d_pixels, P.n_pixels, P.pass_spp, c->stream));
	}
	HIP_TRY(s_albedo.copy_back(c));
	HIP_TRY(s_normal.copy_back(c));
	if (stats || !dev_out) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) return f.stats(c, rays, stats);
	return PTX_OK;
}

}  // namespace

int ptx_render_aov(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_aov_buffers* out, ptx_render_stats* stats) {
	// every refusal, here and in aov_frame, is decided before any device work
	if (!sc || !cfg || !out) return set_err(PTX_ERR_INVALID, "ptx_render_aov: NULL argument");
	if (!out->albedo_cov && !out->normal_depth) return set_err(PTX_ERR_INVALID, "ptx_render_aov: both buffers are NULL (at least one must be given)");
	return aov_frame(sc, cfg, "ptx_render_aov", out->albedo_cov, out->normal_depth, AovKind::guides, nullptr, stats);
}

int ptx_render_motion(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_motion_prev* prev, float* motion, ptx_render_stats* stats) {
	// every refusal, here and in aov_frame, is decided before any device work
	auto bad = [](const char* m) { return set_err(PTX_ERR_INVALID, std::string("ptx_render_motion: ") + m); };
	if (!sc || !cfg || !motion) return bad("NULL argument");
	if (prev && prev->model_xform) {
		const size_t n_models = sc->host.model_xform.size() / 12;   // the size never changes after creation
		if (prev->n_models != n_models) return bad("n_models differs from the scene's");
		for (size_t k = 0; k < 12 * n_models; k++)
			if (!std::isfinite(prev->model_xform[k])) return bad("a previous transform value is not finite");
	}
	if (prev && prev->camera) {   // what ptx_scene_set_camera refuses of a pinhole camera; the lens fields are ignored
		const ptx_camera& pc = *prev->camera;
		for (int k = 0; k < 3; k++) if (!std::isfinite(pc.origin[k])) return bad("the previous camera's origin is not finite");
		for (int k = 0; k < 9; k++) if (!std::isfinite(pc.basis[k])) return bad("the previous camera's basis is not finite");
		if (!std::isfinite(pc.yfov) || !(pc.yfov > 0) || !((double)pc.yfov < 3.14159265358979323846)) return bad("the previous camera's yfov must lie in (0, pi)");
	}
	return aov_frame(sc, cfg, "ptx_render_motion", motion, nullptr, AovKind::motion, prev, stats);
}

int ptx_render_emission(ptx_scene* sc, const ptx_render_cfg* cfg, float* emission, ptx_render_stats* stats) {
	// every refusal, here and in aov_frame, is decided before any device work
	if (!sc || !cfg || !emission) return set_err(PTX_ERR_INVALID, "ptx_render_emission: NULL argument");
	return aov_frame(sc, cfg, "ptx_render_emission", emission, nullptr, AovKind::emission, nullptr, stats);
}

int punctual_on_device_locked(ptx_scene* sc, NeePunctual& Pn) {
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> tl(sc->lights_mu);
	ptx_scene::Punctual& pl = sc->punctual;
	if (pl.cdf.empty()) return PTX_OK;
	if (!pl.on_device) {
		HIP_TRY(sc->d_punctual.ensure(pl.recs.size() * 4));
		HIP_TRY(sc->d_punctual_cdf.ensure(pl.cdf.size() * 4));
		HIP_TRY(hipMemcpyAsync(sc->d_punctual.p, pl.recs.data(), pl.recs.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(sc->d_punctual_cdf.p, pl.cdf.data(), pl.cdf.size() * 4, hipMemcpyHostToDevice, c->stream));
		if (!pl.tree.empty()) {
			HIP_TRY(sc->d_punctual_tree.ensure(pl.tree.size() * 4));
			HIP_TRY(hipMemcpyAsync(sc->d_punctual_tree.p, pl.tree.data(), pl.tree.size() * 4, hipMemcpyHostToDevice, c->stream));
		}
		HIP_TRY(hipStreamSynchronize(c->stream));
		pl.on_device = true;
	}
	Pn.recs = (const float4*)sc->d_punctual.p; Pn.cdf = (const float*)sc->d_punctual_cdf.p; Pn.n = (uint32_t)pl.cdf.size();
	if (!pl.tree.empty()) { Pn.nodes = (const float4*)sc->d_punctual_tree.p; Pn.n_nodes = (uint32_t)(pl.tree.size() / 8); }   // tree mode
	return PTX_OK;
}

int lights_on_device_locked(ptx_scene* sc, NeeLights& Lt) {
	ptx_ctx* c = sc->ctx;
	const ptx_scene::LightList& ll = *build_lights(sc);
	const uint32_t n_lights = (uint32_t)ll.cdf.size();
	if (!n_lights) return PTX_OK;
	if (!ll.tree.empty() && ll.cdf.size() > ((size_t)1 << 30))
		return set_err(PTX_ERR_UNSUPPORTED, "the light tree (PTX_LIGHT_PICK_TREE) holds at most 2^30 listed triangles: a path word has 32 bits");
	if (!sc->lights.on_device) {
		HIP_TRY(sc->d_light_tris.ensure(ll.tris.size() * 4));
		HIP_TRY(sc->d_light_cdf.ensure(ll.cdf.size() * 4));
		HIP_TRY(sc->d_light_geom.ensure(ll.geom.size() * 4));
		HIP_TRY(sc->d_light_first.ensure(ll.surf_first.size() * 4));
		HIP_TRY(hipMemcpyAsync(sc->d_light_tris.p, ll.tris.data(), ll.tris.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(sc->d_light_cdf.p, ll.cdf.data(), ll.cdf.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(sc->d_light_geom.p, ll.geom.data(), ll.geom.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(sc->d_light_first.p, ll.surf_first.data(), ll.surf_first.size() * 4, hipMemcpyHostToDevice, c->stream));
		if (!ll.tree.empty()) {   // tree mode: the tree and the path words travel with the list
			HIP_TRY(sc->d_light_tree.ensure(ll.tree.size() * 4));
			HIP_TRY(sc->d_light_path.ensure(ll.path.size() * 4));
			HIP_TRY(hipMemcpyAsync(sc->d_light_tree.p, ll.tree.data(), ll.tree.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipMemcpyAsync(sc->d_light_path.p, ll.path.data(), ll.path.size() * 4, hipMemcpyHostToDevice, c->stream));
		}
		HIP_TRY(hipStreamSynchronize(c->stream));
		sc->lights.on_device = true;
	}
	Lt.tris = (const uint2*)sc->d_light_tris.p; Lt.cdf = (const float*)sc->d_light_cdf.p; Lt.geom = (const float4*)sc->d_light_geom.p;
	Lt.surf_first = (const int32_t*)sc->d_light_first.p; Lt.n = n_lights; Lt.area = ll.area;
	if (!ll.tree.empty()) { Lt.nodes = (const float4*)sc->d_light_tree.p; Lt.path = (const uint32_t*)sc->d_light_path.p; Lt.n_nodes = (uint32_t)(ll.tree.size() / 8); }
	return PTX_OK;
}

namespace {

// What ptx_render_nee's passes read besides the scene: the light list and the environment table on the device, and which form renders.
// Made once per call (nee_setup_locked); ptx_render_adaptive_nee shares one over its rounds.
struct NeeSetup {
	NeeLights Lt{};
	NeeEnv Ev{};
	NeePunctual Pn{};        // the scene's punctual lights; n != 0: the PUN variants run
	uint32_t n_lights = 0;   // listed triangles, whatever the flags
	float light_area = 0;
	bool fused = false;      // PTX_NEE_FUSED on a scene of the fused route; under active motion only with PTX_NEE_FUSED_MOTION beside it
	bool sampler_pdf = false;   // PTX_NEE_SAMPLER_PDF where a light sample is possible
	uint32_t candidates = 1;    // M of PTX_NEE_CANDIDATES where a light sample is possible; above 1 the RIS variants run
};
// Where a pass's samples go. b == nullptr: all of them into a (k_resolve). Otherwise the call's samples [0, split) into a and the rest into b
// (k_resolve_halves): pass p, whose first sample is p * pass_spp, gives a its first clamp(split - p * pass_spp, 0, samples of the pass).
struct NeeTargets {
	float4 *a, *b;
	uint32_t split;
};

hipError_t nee_resolve(const float4* rad, const NeeTargets& T, const PassFrame& f, const RenderParams& P, uint32_t p, hipStream_t stream) {
	if (!T.b) return launch_resolve(rad, T.a, f.d_pixels, P.n_pixels, P.pass_spp, stream);
	const int64_t left = (int64_t)T.split - (int64_t)p * f.pass_spp;
	const uint32_t n_a = (uint32_t)std::clamp<int64_t>(left, 0, (int64_t)P.pass_spp);
	return launch_resolve_halves(rad, T.a, T.b, f.d_pixels, P.n_pixels, P.pass_spp, n_a, stream);
}

// The light list and, for PTX_NEE_ENV_SAMPLES, the environment table: built and uploaded at the first call that asks, then kept on the scene.
// The caller holds the context's mutex and has set the device.
int nee_setup_locked(ptx_scene* sc, uint32_t flags, NeeSetup& S) {
	ptx_ctx* c = sc->ctx;
	const ptx_scene::LightList& ll = *build_lights(sc);
	const uint32_t n_lights = (uint32_t)ll.cdf.size();
	S.n_lights = n_lights; S.light_area = ll.area;
	// PTX_NEE_FUSED: one launch per pass wherever ptx_render would run the fused kernel; a scene of the queue route renders as without the flag
	// ... and under active motion it is ignored, not refused, unless PTX_NEE_FUSED_MOTION stands beside it: then the fused kernel that carries a
	// time per lane runs (nee_fused_motion.hip). PTX_NEE_FUSED_MOTION without PTX_NEE_FUSED, or without active motion, changes nothing.
	S.fused = (flags & PTX_NEE_FUSED) != 0 && !use_wavefront(sc) && (!motion_active(sc) || (flags & PTX_NEE_FUSED_MOTION) != 0);
	if (n_lights && !(flags & PTX_NEE_NO_LIGHT_SAMPLES)) {
		if (const int rc = lights_on_device_locked(sc, S.Lt); rc != PTX_OK) return rc;
		// Tree mode with a non-empty list under active motion (include/ptx.h: LIGHT PICK, FORMS): k_nee_fused_motion has no tree variants,
		// so PTX_NEE_FUSED | PTX_NEE_FUSED_MOTION is ignored as PTX_NEE_FUSED alone is, and the unfused form renders the tree
		if (S.Lt.nodes && motion_active(sc)) S.fused = false;
	}
	// PTX_NEE_ENV_SAMPLES: the ENV variants wherever the map has a table; no map or a black one: the call runs exactly as without the flag
	if (flags & PTX_NEE_ENV_SAMPLES) {
		const ptx_scene::EnvTable& et = *build_env_table(sc);
		if (!et.row_cdf.empty() && sc->dev.env_tex >= 0) {
			if (!sc->env_table.on_device) {
				HIP_TRY(sc->d_env_row.ensure(et.row_cdf.size() * 4));
				HIP_TRY(sc->d_env_cell.ensure(et.cell_cdf.size() * 4));
				HIP_TRY(hipMemcpyAsync(sc->d_env_row.p, et.row_cdf.data(), et.row_cdf.size() * 4, hipMemcpyHostToDevice, c->stream));
				HIP_TRY(hipMemcpyAsync(sc->d_env_cell.p, et.cell_cdf.data(), et.cell_cdf.size() * 4, hipMemcpyHostToDevice, c->stream));
				HIP_TRY(hipStreamSynchronize(c->stream));
				sc->env_table.on_device = true;
			}
			NeeEnv& Ev = S.Ev;
			Ev.row_cdf = (const float*)sc->d_env_row.p; Ev.cell_cdf = (const float*)sc->d_env_cell.p; Ev.w = et.w; Ev.h = et.h;
		}
	}
	// punctual lights on the scene: a third kind of candidate, whatever the flags. The copy goes up at the first call after a set.
	if (const int rc = punctual_on_device_locked(sc, S.Pn); rc != PTX_OK) return rc;
	// PTX_NEE_SAMPLER_PDF changes weights only: with no light sample that has a weight possible every weight is 1, and the unflagged variants
	// run (a punctual sample has none: alone it leaves every weight 1)
	S.sampler_pdf = (flags & PTX_NEE_SAMPLER_PDF) != 0 && (S.Lt.n != 0 || S.Ev.row_cdf != nullptr);
	// PTX_NEE_CANDIDATES: with no light sample possible no candidate is drawn, and the unflagged variants run
	S.candidates = (S.Lt.n != 0 || S.Ev.row_cdf != nullptr || S.Pn.n != 0) ? ((flags >> 8) & 15u) + 1u : 1u;
	return PTX_OK;
}

// ptx_render_nee with PTX_NEE_FUSED on a scene of the fused route: one launch of k_nee_fused per pass (under active motion, which only
// PTX_NEE_FUSED_MOTION lets come here: of k_nee_fused_motion), then the resolve. No round trips to the
// host and no streams: the workspace is ptx_render's radiance records, overflow stacks and counters. The caller holds the context's mutex, has
// set the device, planned the passes and made the setup. With stats the stream is synchronised.
int nee_fused_frame(ptx_ctx* c, ptx_scene* sc, const PassFrame& f, const NeeSetup& S, const NeeTargets& T, ptx_nee_stats* stats) {
	const int grid = c->n_cu;
	HIP_TRY(c->sample_rad.ensure((size_t)f.pass_spp * f.n_pixels * sizeof(float4)));
	HIP_TRY(c->counters.ensure(1024));   // [0] chunk counter, [16] rays, [24] light samples, [32] visible light samples
	HIP_TRY(c->spill.ensure((size_t)grid * (kBlock / 64) * (size_t)kSpillWords * sizeof(uint2)));
	HIP_TRY(hipMemsetAsync(c->counters.p, 0, 1024, c->stream));
	const NeeFusedBuffers B{(float4*)c->sample_rad.p, (uint2*)c->spill.p, (unsigned long long*)c->counters.p, (unsigned long long*)((char*)c->counters.p + 16)};
	const RenderMotion Rm = render_motion(sc);   // what the unfused form's kernels take
	if (stats)
		if (const int rc = PassFrame::ensure_events(c, f.n_pass); rc != PTX_OK) return rc;
	for (uint32_t p = 0; p < f.n_pass; p++) {
		RenderParams P = f.params(p, true);
		P.integrator = PTX_INTEGRATOR_LIB;
		HIP_TRY(hipMemsetAsync(B.chunk_counter, 0, 8, c->stream));
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		if (Rm.active) HIP_TRY(launch_nee_fused_motion(sc->dev, P, S.Lt, S.Ev, S.Pn, S.sampler_pdf, S.candidates, Rm, B, sc->mode, sc->lds_bytes, grid, c->stream));
		else HIP_TRY(launch_nee_fused(sc->dev, P, S.Lt, S.Ev, S.Pn, S.sampler_pdf, S.candidates, B, sc->mode, sc->lds_bytes, grid, c->stream));
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		HIP_TRY(nee_resolve(B.sample_rad, T, f, P, p, c->stream));
	}
	if (stats) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		unsigned long long cnt[3] = {0, 0, 0};   // rays, light samples, visible ones
		HIP_TRY(hipMemcpy(cnt, B.counters, sizeof cnt, hipMemcpyDeviceToHost));
		stats->light_samples = cnt[1]; stats->light_visible = cnt[2];
		if (const int rc = f.stats(c, cnt[0], &stats->render); rc != PTX_OK) return rc;
		c->timing.pipeline = 0u;
		c->timing.workspace_bytes = c->spill.cap;
		c->timing.fused_ms = stats->render.kernel_ms;
		c->timing.fused_launches = f.n_pass;
	}
	return PTX_OK;
}

// The passes of one ptx_render_nee call — the samples [cfg->sample0, cfg->sample0 + cfg->spp) of cfg's rectangle, or of `subset`'s pixels of
// it — into the DEVICE buffers of `T`. The caller holds the context's mutex, has set the device, checked cfg and made the setup. With stats
// (zeroed here, and the context's timing with them) the stream is synchronised; without, nothing waits for the last pass.
int nee_frame_locked(ptx_scene* sc, const ptx_render_cfg* cfg, const char* who, const NeeSetup& S, const NeeTargets& T, const PixelSubset* subset, ptx_nee_stats* stats) {
	PassFrame f;
	f.cfg = cfg;
	if (const int rc = render_rect(cfg, who, true, f.x0, f.y0, f.w, f.h); rc != PTX_OK) return rc;
	ptx_ctx* c = sc->ctx;
	if (stats) {
		*stats = ptx_nee_stats{}; c->timing = ptx_kernel_timing{}; c->timing.pipeline = use_wavefront(sc) ? 1u : 0u;
		stats->n_lights = S.n_lights; stats->light_area = S.light_area;
	}
	// The wavefront form's workspace takes 68 words per sample (74 in tree mode: x_prev beside both streams), so by default a pass has 16 Mi samples (8 spp of a 1080p frame, 4.6 GB); at most
	// 2^30, so that the positions of a round's shadow rays (two per path at most) stay below 2^31. The fused form keeps only the 16-byte
	// radiance record per sample: ptx_render's pass size and id limit.
	if (const int rc = f.plan(c, sc, who, subset, S.fused ? 128ull << 20 : 16ull << 20, S.fused ? 0xFFFFFFFFull : 0x3FFFFFFFull); rc != PTX_OK || !f.n_pass) return rc;
	if (S.fused) return nee_fused_frame(c, sc, f, S, T, stats);
	const NeeLights& Lt = S.Lt;
	const NeeEnv& Ev = S.Ev;

	// workspace of one pass of `cap` samples: [256 B: counters][radiance records][stream 0][stream 1][hits][shadow rays][shadow hits][shadow records]
	const size_t cap = ((size_t)f.pass_spp * f.n_pixels + 3) & ~(size_t)3;   // array stride: keeps every array 16-byte aligned
	uint32_t* cnt = nullptr;
	float4* Lrec = nullptr;
	NeeStream st[2];
	NeePrev prev[2] = {};
	float *hits = nullptr, *shits = nullptr;
	NeeShadow W{};
	const RenderMotion Rm = render_motion(sc);
	const bool tree = Lt.n != 0 && Lt.nodes != nullptr;   // the LTREE variants run: the streams carry x_prev
	float* times = nullptr;   // under motion of a model: the time of each path ray of the round, in stream order; the shadow rays' are W.tm
	auto carve = [&](void* base) {
		Carver k(base);
		cnt = k.take<uint32_t>(64);
		Lrec = k.take<float4>(cap);
		for (NeeStream& s : st) {
			s.ox = k.take<float>(cap); s.oy = k.take<float>(cap); s.oz = k.take<float>(cap);
			s.dx = k.take<float>(cap); s.dy = k.take<float>(cap); s.dz = k.take<float>(cap);
			s.tx = k.take<float>(cap); s.ty = k.take<float>(cap); s.tz = k.take<float>(cap); s.pp = k.take<float>(cap);
			s.id = k.take<uint32_t>(cap); s.dp = k.take<uint32_t>(cap);
		}
		for (NeePrev& x : prev)   // x_prev beside each stream: tree mode alone
			if (tree) { x.px = k.take<float>(cap); x.py = k.take<float>(cap); x.pz = k.take<float>(cap); }
		hits = k.take<float>(6 * cap);
		W.ox = k.take<float>(2 * cap); W.oy = k.take<float>(2 * cap); W.oz = k.take<float>(2 * cap);
		W.dx = k.take<float>(2 * cap); W.dy = k.take<float>(2 * cap); W.dz = k.take<float>(2 * cap);
		shits = k.take<float>(12 * cap);
		W.sx = k.take<float>(cap); W.sy = k.take<float>(cap); W.sz = k.take<float>(cap);
		W.lx = k.take<float>(cap); W.ly = k.take<float>(cap); W.lz = k.take<float>(cap);
		W.sun_pos = k.take<uint32_t>(cap); W.light_pos = k.take<uint32_t>(cap); W.exp_surf = k.take<uint32_t>(cap); W.exp_tri = k.take<uint32_t>(cap);
		times = k.take<float>(Rm.models_moved ? cap : 0);
		W.tm = k.take<float>(Rm.active ? 2 * cap : 0);
		return k.off;
	};
	HIP_TRY(c->round_ws.ensure(carve(nullptr)));
	carve(c->round_ws.p);

	if (stats)
		if (const int rc = PassFrame::ensure_events(c, f.n_pass); rc != PTX_OK) return rc;
	HIP_TRY(hipMemsetAsync(cnt, 0, 256, c->stream));
	// a lit shadow catcher's pass-through ray is appended by the settle kernel: only then is the live count read a second time in a round
	const bool catchers = sc->dev.any_alpha != 0 && sc->dev.sun.present != 0;
	uint64_t rays = 0;
	for (uint32_t p = 0; p < f.n_pass; p++) {
		RenderParams P = f.params(p, true);
		P.integrator = PTX_INTEGRATOR_LIB;
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		HIP_TRY(launch_nee_generate(sc->dev, P, st[0], Lrec, (uint32_t)P.n_paths, Rm, c->stream));
		uint32_t live = P.bounces > 0 ? (uint32_t)P.n_paths : 0u;
		for (uint32_t round = 0; live != 0; round++) {
			const NeeStream& in = st[round & 1u];
			const NeeStream& out = st[(round + 1u) & 1u];
			IntersectArgs A{};
			A.n = live;
			ray_args(A, in.ox, cap);
			hit_args(A, hits, cap);
			if (Rm.models_moved) {   // a time per ray: the sample's, whichever round its path is in
				HIP_TRY(launch_motion_times(P, Rm, in.id, live, times, c->stream));
				A.time = times;
				A.motion = Rm.models;
			}
			if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
			rays += live;
			const NeeHits H{A.distance, A.surface, A.triangle, A.b1, A.b2};
			HIP_TRY(hipMemsetAsync(cnt, 0, 8, c->stream));
			HIP_TRY(launch_nee_shade(sc->dev, P, Lt, Ev, S.Pn, S.sampler_pdf, S.candidates, in, H, live, out, W, cnt, Lrec, Rm, prev[round & 1u], prev[(round + 1u) & 1u], c->stream));
			uint32_t got[2] = {0, 0};   // continuations, shadow rays
			HIP_TRY(hipMemcpyAsync(got, cnt, 8, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			if (got[0] > live || got[1] > 2ull * live) return set_err(PTX_ERR_HIP, std::string(who) + ": a round appended more entries than its paths allow");
			if (got[1]) {
				IntersectArgs B{};
				B.n = got[1];
				ray_args(B, W.ox, 2 * cap);
				hit_args(B, shits, 2 * cap);
				if (Rm.models_moved) { B.time = W.tm; B.motion = Rm.models; }   // k_nee_shade wrote each shadow ray's time beside it
				if (const int rc = intersect_device(c, sc, B); rc != PTX_OK) return rc;
				rays += got[1];
				const NeeHits SH{B.distance, B.surface, B.triangle, B.b1, B.b2};
				HIP_TRY(launch_nee_settle(in, live, W, SH, out, cnt, Lrec, S.Pn.n != 0, prev[round & 1u], prev[(round + 1u) & 1u], c->stream));
				if (catchers) {
					HIP_TRY(hipMemcpyAsync(got, cnt, 4, hipMemcpyDeviceToHost, c->stream));
					HIP_TRY(hipStreamSynchronize(c->stream));
					if (got[0] > live) return set_err(PTX_ERR_HIP, std::string(who) + ": a round appended more entries than its paths allow");
				}
			}
			live = got[0];
		}
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		HIP_TRY(nee_resolve(Lrec, T, f, P, p, c->stream));
	}
	if (stats) {
		HIP_TRY(hipStreamSynchronize(c->stream));
		unsigned long long ls[2] = {0, 0};
		HIP_TRY(hipMemcpy(ls, cnt + 2, 16, hipMemcpyDeviceToHost));
		stats->light_samples = ls[0]; stats->light_visible = ls[1];
		return f.stats(c, rays, &stats->render);
	}
	return PTX_OK;
}

constexpr uint32_t kNeeFlags = PTX_NEE_NO_LIGHT_SAMPLES | PTX_NEE_FUSED | PTX_NEE_ENV_SAMPLES | PTX_NEE_SAMPLER_PDF | PTX_NEE_CANDIDATES(16) | PTX_NEE_FUSED_MOTION;   // bits 8..11: the candidate count

}  // namespace

int ptx_render_nee(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_nee_cfg* ncfg, float* accum, ptx_nee_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !accum) return set_err(PTX_ERR_INVALID, "ptx_render_nee: NULL argument");
	const uint32_t flags = ncfg ? ncfg->flags : 0u;
	if (flags & ~kNeeFlags) return set_err(PTX_ERR_INVALID, "ptx_render_nee: unknown flag");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_nee: PTX_INTEGRATOR_WORKER has no light sampling here (the estimator is defined on PTX_INTEGRATOR_LIB's vertex)");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_nee: scene was created without a GPU context (no CPU path exists)");
	uint32_t x0, y0, w, h;
	if (const int rc = render_rect(cfg, "ptx_render_nee", true, x0, y0, w, h); rc != PTX_OK) return rc;
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	NeeSetup S;
	if (const int rc = nee_setup_locked(sc, flags, S); rc != PTX_OK) return rc;
	const bool dev_accum = is_device_ptr(accum);
	Staged s_accum;
	if (cfg->spp) HIP_TRY(s_accum.bind(c, dev_accum, accum, (size_t)w * h * sizeof(float4), c->stage_a));
	if (const int rc = nee_frame_locked(sc, cfg, "ptx_render_nee", S, NeeTargets{s_accum.as<float4>(), nullptr, 0u}, nullptr, stats); rc != PTX_OK) return rc;
	if (cfg->spp) HIP_TRY(s_accum.copy_back(c));
	if (cfg->spp && !dev_accum) HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

namespace {

// What ptx_render_adaptive and ptx_render_adaptive_nee refuse in their arguments with PTX_ERR_INVALID, decided before any device work;
// -> the rectangle and the round size
int adaptive_args(const char* who, const void* sc, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, const float* accum_a, const float* accum_b, uint32_t& x0, uint32_t& y0,
                  uint32_t& w, uint32_t& h, uint32_t& step) {
	auto bad = [who](const char* m) { return set_err(PTX_ERR_INVALID, std::string(who) + ": " + m); };
	if (!sc || !cfg || !acfg || !accum_a || !accum_b) return bad("NULL argument");
	if (acfg->min_spp < 2 || (acfg->min_spp & 1u)) return bad("min_spp must be even and >= 2 (each round is split into two halves)");
	if (acfg->step_spp & 1u) return bad("step_spp must be even (0 = min_spp)");
	if ((cfg->spp & 1u) || cfg->spp < acfg->min_spp) return bad("spp (the cap) must be even and >= min_spp");
	step = acfg->step_spp ? acfg->step_spp : acfg->min_spp;
	if ((uint64_t)1 + ((uint64_t)(cfg->spp - acfg->min_spp) + step - 1) / step > 4096) return bad("more than 4096 rounds");
	if (!(acfg->threshold >= 0.0f)) return bad("threshold is negative or NaN");
	if ((uint64_t)cfg->sample0 + cfg->spp > 0xFFFFFFFFull) return bad("sample0 + spp overflows");
	if (const int rc = render_rect(cfg, who, true, x0, y0, w, h); rc != PTX_OK) return rc;
	if (w > kAdMaxSide || h > kAdMaxSide) return bad("the rectangle's sides must be at most 16384");
	return PTX_OK;
}

// The refusal of shard_count > 1 on a scene without a context, where no exchange can be registered; with one the registration is looked at
// under its lock (adaptive_loop).
std::string no_exchange(const char* who) {
	return std::string(who) + ": shard_count > 1 needs a mask exchange (the 3 x 3 block of the decision reads the noisy bytes of pixels that other shards own): register one "
	       "with ptx_ctx_set_mask_exchange, and the shards' buffers sum to the unsharded frame bit for bit, which rectangles decided on their own do not";
}

struct AdaptiveRun {
	uint32_t rounds = 0, active_last = 0;
	double select_ms = 0;
};

// What ptx_render_adaptive and ptx_render_adaptive_nee share: the half-buffers staged once, the `done` bytes and the active list, the round
// sizes, the decision after every round, the sharded form of it, the copy back. render_round(round_cfg, given, k, subset, d_a, d_b) adds
// the samples [sample0 + given, sample0 + given + k) of the subset's pixels (nullptr: pixel_list()'s, which honours shard_*) to the two
// halves; round_cfg holds the validated rectangle. The caller holds the context's mutex; the device is set here, after the last refusal.
template <class RenderRound>
int adaptive_loop(ptx_scene* sc, const char* who, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t step,
                  float* accum_a, float* accum_b, bool dev, bool want_ms, RenderRound&& render_round, AdaptiveRun& run) {
	ptx_ctx* c = sc->ctx;
	const size_t n = (size_t)w * h, bytes = n * sizeof(float4);
	ptx_ctx::MaskExchange& X = c->mask_exchange;
	const bool sharded = cfg->shard_count > 1;
	AdaptiveShard shard{};
	if (sharded) {
		if (!X.fn) return set_err(PTX_ERR_UNSUPPORTED, no_exchange(who));
		if (X.bytes < n) return set_err(PTX_ERR_INVALID, std::string(who) + ": the mask of ptx_ctx_set_mask_exchange is smaller than w * h bytes of the rectangle");
		const uint32_t ts = cfg->shard_tile ? cfg->shard_tile : 64u;
		shard = AdaptiveShard{x0, y0, ts, (cfg->W + ts - 1) / ts, cfg->shard_index, cfg->shard_count};
		if ((uint64_t)shard.tiles_x * ((cfg->H + ts - 1) / ts) > 0xFFFFFFFFull) return set_err(PTX_ERR_INVALID, std::string(who) + ": more than 2^32 - 1 shard tiles in the image");
	}
	X.calls = 0;
	X.wall_ms = 0;
	HIP_TRY(hipSetDevice(c->device));
	const bool mask_on_device = sharded && is_device_ptr(X.mask);

	Staged s_a, s_b;   // staged once for the whole call, both in one buffer
	if (!dev) HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
	HIP_TRY(s_a.bind(c, dev, accum_a, bytes, c->adaptive_stage));
	HIP_TRY(s_b.bind(c, dev, accum_b, bytes, c->adaptive_stage, bytes));
	float4 *const d_a = s_a.as<float4>(), *const d_b = s_b.as<float4>();
	HIP_TRY(c->adaptive_state.ensure(n * 4 + pad16(n)));
	uint32_t* const d_list = (uint32_t*)c->adaptive_state.p;
	uint8_t* const d_done = (uint8_t*)c->adaptive_state.p + n * 4;
	HIP_TRY(hipMemsetAsync(d_done, 0, n, c->stream));

	ptx_render_cfg round = *cfg;
	round.x0 = x0; round.y0 = y0; round.w = w; round.h = h;
	PixelSubset active{d_list, 0};
	uint32_t given = 0, n_active = 0, n_all = 0;
	while (given < cfg->spp) {
		const uint32_t k = run.rounds == 0 ? acfg->min_spp : std::min(step, cfg->spp - given);   // even: min_spp, step_spp and the cap are
		// a rank that owns no active pixel renders nothing in this round and still takes part in the exchange
		if (run.rounds == 0 || active.n_pixels)
			if (const int rc = render_round(round, given, k, run.rounds == 0 ? nullptr : &active, d_a, d_b); rc != PTX_OK) return rc;
		given += k;
		run.rounds++;
		if (sharded) {
			bool exchange_failed = false;
			if (const int rc = adaptive_decide_sharded_locked(c, w, h, shard, mask_on_device, d_a, d_b, acfg->threshold, d_done, d_list, n_active, n_all, want_ms ? &run.select_ms : nullptr,
			                                                  exchange_failed);
			    rc != PTX_OK) {
				if (exchange_failed && !dev) {   // the buffers hold the completed rounds
					const std::string msg = ptx_last_error();
					if (s_a.copy_back(c) == hipSuccess && s_b.copy_back(c) == hipSuccess) (void)hipStreamSynchronize(c->stream);
					return set_err(rc, msg);
				}
				return rc;
			}
		} else {
			if (const int rc = adaptive_decide_locked(c, w, h, d_a, d_b, acfg->threshold, d_done, d_list, n_active, want_ms ? &run.select_ms : nullptr); rc != PTX_OK) return rc;
			n_all = n_active;
		}
		active.n_pixels = n_active;
		if (n_all == 0) break;
	}
	HIP_TRY(s_a.copy_back(c));
	HIP_TRY(s_b.copy_back(c));
	if (!dev) HIP_TRY(hipStreamSynchronize(c->stream));
	run.active_last = n_active;
	return PTX_OK;
}

}  // namespace

int ptx_render_adaptive(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, float* accum_a, float* accum_b, ptx_adaptive_stats* stats) {
	// every refusal below is decided before any device work
	uint32_t x0, y0, w, h, step;
	if (const int rc = adaptive_args("ptx_render_adaptive", sc, cfg, acfg, accum_a, accum_b, x0, y0, w, h, step); rc != PTX_OK) return rc;
	if (motion_active(sc)) return refuse_motion("ptx_render_adaptive");
	if (cfg->shard_count > 1 && !sc->ctx) return set_err(PTX_ERR_UNSUPPORTED, no_exchange("ptx_render_adaptive"));
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_adaptive: scene was created without a GPU context (no CPU path exists)");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: accum_a and accum_b must both be device or both be host memory");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	if (stats) *stats = ptx_adaptive_stats{};

	// the first half of the round's samples into A, the second into B: one sequence of passes each
	auto render_round = [&](ptx_render_cfg& half, uint32_t given, uint32_t k, const PixelSubset* subset, float4* d_a, float4* d_b) {
		float4* const target[2] = {d_a, d_b};
		for (uint32_t part = 0; part < 2; part++) {
			half.sample0 = cfg->sample0 + given + part * (k / 2);
			half.spp = k / 2;
			ptx_render_stats st{};
			if (const int rc = render_frame_locked(sc, &half, "ptx_render_adaptive", (float*)target[part], nullptr, stats ? &st : nullptr, subset); rc != PTX_OK) return rc;
			if (stats) {
				stats->render.rays += st.rays; stats->render.samples += st.samples; stats->render.passes += st.passes; stats->render.kernel_ms += st.kernel_ms;
			}
		}
		return (int)PTX_OK;
	};
	AdaptiveRun run;
	if (const int rc = adaptive_loop(sc, "ptx_render_adaptive", cfg, acfg, x0, y0, w, h, step, accum_a, accum_b, dev, stats != nullptr, render_round, run); rc != PTX_OK) return rc;
	if (stats) {
		stats->rounds = run.rounds;
		stats->active_last = run.active_last;
		stats->select_ms = run.select_ms;
	}
	return PTX_OK;
}

// ptx_render_adaptive's loop on ptx_render_nee's estimator. A round is ONE sequence of passes over its k samples, resolved into both halves
// (k_resolve_halves: the first k / 2 samples into A, the rest into B), not one sequence per half: half the launches' fixed price per round.
int ptx_render_adaptive_nee(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, const ptx_nee_cfg* ncfg, float* accum_a, float* accum_b,
                            ptx_adaptive_nee_stats* stats) {
	// every refusal below is decided before any device work
	uint32_t x0, y0, w, h, step;
	if (const int rc = adaptive_args("ptx_render_adaptive_nee", sc, cfg, acfg, accum_a, accum_b, x0, y0, w, h, step); rc != PTX_OK) return rc;
	const uint32_t flags = ncfg ? ncfg->flags : 0u;
	if (flags & ~kNeeFlags) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive_nee: unknown flag");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_adaptive_nee: PTX_INTEGRATOR_WORKER has no light sampling here (the estimator is defined on PTX_INTEGRATOR_LIB's vertex)");
	if (cfg->shard_count > 1 && !sc->ctx) return set_err(PTX_ERR_UNSUPPORTED, no_exchange("ptx_render_adaptive_nee"));
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_adaptive_nee: scene was created without a GPU context (no CPU path exists)");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive_nee: accum_a and accum_b must both be device or both be host memory");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	if (stats) *stats = ptx_adaptive_nee_stats{};

	NeeSetup S;   // the light list and the environment table: once for all rounds, made by the first round
	bool have_setup = false;
	ptx_kernel_timing timing{};
	// PTX_ADAPTIVE_NEE_HALVES=1 (measurement, tools/bench_adaptive.py): every round as ptx_render_adaptive drives it, one sequence of passes per
	// half through k_resolve. The same bits; twice the launches. What the one-sequence form saves is the difference.
	const char* const halves_env = getenv("PTX_ADAPTIVE_NEE_HALVES");
	const bool two_sequences = halves_env && halves_env[0] == '1';
	auto render_round = [&](ptx_render_cfg& round, uint32_t given, uint32_t k, const PixelSubset* subset, float4* d_a, float4* d_b) {
		if (!have_setup) {
			if (const int rc = nee_setup_locked(sc, flags, S); rc != PTX_OK) return rc;
			have_setup = true;
		}
		// one sequence of passes over the round's k samples, resolved into both halves; under the measurement switch one sequence per half
		for (uint32_t part = 0; part < (two_sequences ? 2u : 1u); part++) {
			round.sample0 = cfg->sample0 + given + part * (k / 2);
			round.spp = two_sequences ? k / 2 : k;
			const NeeTargets T = two_sequences ? NeeTargets{part ? d_b : d_a, nullptr, 0u} : NeeTargets{d_a, d_b, k / 2};
			ptx_nee_stats st{};
			if (const int rc = nee_frame_locked(sc, &round, "ptx_render_adaptive_nee", S, T, subset, stats ? &st : nullptr); rc != PTX_OK) return rc;
			if (stats) {
				ptx_nee_stats& t = stats->nee;
				t.render.rays += st.render.rays; t.render.samples += st.render.samples; t.render.passes += st.render.passes; t.render.kernel_ms += st.render.kernel_ms;
				t.light_samples += st.light_samples; t.light_visible += st.light_visible;
				timing.pipeline = c->timing.pipeline;
				timing.workspace_bytes = std::max(timing.workspace_bytes, c->timing.workspace_bytes);
				timing.fused_ms += c->timing.fused_ms;
				timing.fused_launches += c->timing.fused_launches;
			}
		}
		return (int)PTX_OK;
	};
	AdaptiveRun run;
	if (const int rc = adaptive_loop(sc, "ptx_render_adaptive_nee", cfg, acfg, x0, y0, w, h, step, accum_a, accum_b, dev, stats != nullptr, render_round, run); rc != PTX_OK) return rc;
	if (stats) {
		stats->nee.n_lights = S.n_lights;
		stats->nee.light_area = S.light_area;
		stats->rounds = run.rounds;
		stats->active_last = run.active_last;
		stats->select_ms = run.select_ms;
		c->timing = timing;   // the rounds' sums: with the fused form fused_launches == nee.render.passes and fused_ms == nee.render.kernel_ms
	}
	return PTX_OK;
}
