// What the three translation units of the C ABI share (ptx_api.cpp, api_render.cpp, api_batch.cpp): the error slot, the device buffers,
// the context and the scene, and the host plumbing every entry point goes through — staging of caller buffers, the cfg check, pass
// sizing, the pass frame, the workspace carver. Internal: not installed, and nothing declared here is exported from libptx_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ptx.h"
#include "kernels.hpp"

#pragma GCC visibility push(hidden)

using namespace ptx;

// ptx_last_error's thread-local slot (ptx_api.cpp); returns `code`
int set_err(int code, const std::string& m);
#define HIP_TRY(expr)                                                                                           \
	do {                                                                                                        \
		hipError_t e_ = (expr);                                                                                 \
		if (e_ != hipSuccess) return set_err(PTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
	} while (0)

inline bool is_device_ptr(const void* p) {
	hipPointerAttribute_t a;
	hipError_t e = hipPointerGetAttributes(&a, p);
	if (e != hipSuccess) { (void)hipGetLastError(); return false; }
	return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

inline size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

struct DevBuf {
	void* p = nullptr;
	size_t cap = 0;
	hipError_t ensure(size_t bytes) {
		if (bytes <= cap) return hipSuccess;
		if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
		hipError_t e = hipMalloc(&p, bytes);
		if (e == hipSuccess) cap = bytes;
		return e;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct ptx_ctx {
	std::atomic<int> refs{1};   // the caller's handle + one per scene created on it: a scene may outlive ptx_ctx_destroy
	int device = 0;
	hipStream_t stream = nullptr;
	int n_cu = 0;
	std::mutex mu;
	DevBuf queues, sample_rad, counters, spill, stage_a, stage_b, pixel_list, srgb_thr;
	DevBuf round_ws;   // workspace of ptx_render_aov and ptx_render_nee: the streams, hits and per-sample records of one pass
	DevBuf denoise;   // workspace of ptx_denoise: four float4 state buffers per pixel, and the staging of host buffers
	// workspace of ptx_render_adaptive / ptx_adaptive_select: the decision's buffers (noisy bytes, block masks and offsets, tile counts and
	// offsets, the count word), the loop's `done` bytes and active list, and the staging of host buffers
	DevBuf adaptive, adaptive_state, adaptive_stage;
	hipEvent_t adaptive_ev[2] = {nullptr, nullptr};   // around the decision kernels (select_ms)
	// ptx_ctx_set_mask_exchange: the caller's merge of the noisy bytes over the ranks of a sharded adaptive call, and its buffer
	struct MaskExchange {
		ptx_mask_exchange_fn fn = nullptr;
		void* user = nullptr;
		uint8_t* mask = nullptr;
		size_t bytes = 0;
		uint64_t calls = 0;    // of the last adaptive call (ptx_ctx_get_mask_exchange_stats)
		double wall_ms = 0;
	} mask_exchange;
	// workspace of the queue-based pipeline (wavefront.hip): ptx_render and ptx_intersect_batch run it on the context's stream
	struct WfSet {
		DevBuf qent, pair_hit, seg, first, mask, ctl, spill, stream_buf, flow;
		uint32_t* flow_host = nullptr;   // pinned copy of the flow words (kWfFlowWords)
	} wf;
	std::vector<hipEvent_t> events;
	// per-kernel timing of the last ptx_render that was given a stats pointer (ptx_ctx_set_timing / ptx_ctx_get_timing)
	bool timing_on = false;
	std::vector<hipEvent_t> step_events;
	ptx_kernel_timing timing{};
	// pixel list of the last sharded render (ptx_render_cfg::shard_*), kept on the device: a frame is usually rendered again
	// with the same sharding (sample ranges, benchmark steps)
	uint32_t list_key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t list_len = 0;
};

struct ptx_scene {
	ptx_ctx* ctx = nullptr;
	FlatScene host;
	DevBuf d_models, d_surfaces, d_materials, d_nodes, d_refs, d_tris, d_shade, d_tex, d_texels, d_lut, d_spaces, d_model_space, d_wf_order, d_surf_aux;
	DevBuf d_res_nodes, d_res_refs, d_res_tris, d_texels_f, d_hot;
	DevScene dev{};
	double lds_area_share = 0;     // share of the surfaces' box area (sum over surfaces) that belongs to LDS-resident surfaces: how much of what a ray can enter is served from LDS
	double wf_pairs_per_ray = 0;   // queue-based pipeline: pairs (ray, entered surface) per ray seen so far on this scene, 0 = not yet measured
	bool leaf_ordered = true; // global-memory copy of the triangle records: per leaf reference (true) or per triangle (false)
	int kd_shapes = 1;        // shape bits of the leaf-ordered resident trees in SurfaceRec::lds_root (PTX_KD_SHAPES; read with lds_leaf_order)
	int lds_leaf_order = -1;  // LDS-resident copy: leaf-ordered records for the surfaces where they are cheap (1) or all ref-indexed (0); -1 = not decided yet
	size_t lds_budget = 0;    // what plan_residency may fill (decide_mode)
	int mode = MODE_GLOBAL;   // where the traversal arrays live: MODE_GLOBAL / MODE_LDS / MODE_HYBRID (kernels.hip)
	size_t lds_bytes = 0;     // dynamic LDS of the kernels (resident arrays + shade records)
	// The light list of ptx_render_nee (build_lights): built at the first call that asks for it, then kept. Host copies serve
	// ptx_scene_get_array; the device copies are made by the first ptx_render_nee.
	struct LightList {
		bool built = false, on_device = false;
		std::vector<uint32_t> tris;        // [n][2] surface, local triangle
		std::vector<float> cdf, geom;      // [n], [n][4] geometric normal + area
		std::vector<int32_t> surf_first;   // [n_surfaces] first entry or -1
		float area = 0;                    // A_total
		std::vector<uint32_t> tree, path;  // [n_nodes][8], [n] the light tree and each entry's path word (build_light_tree); empty in CDF mode and with an empty list
	} lights;
	uint32_t light_pick = PTX_LIGHT_PICK_CDF;   // ptx_scene_set_light_pick; outlives the list, guarded by lights_mu
	std::mutex lights_mu;   // host-only scenes have no context whose mutex could guard the build
	DevBuf d_light_tris, d_light_cdf, d_light_geom, d_light_first, d_light_tree, d_light_path;
	// The sampling table of the environment map (build_env_table, PTX_NEE_ENV_SAMPLES): built at the first request under lights_mu, dropped
	// by ptx_scene_set_environment. Empty vectors: no map, or a black one. The device copies are made by the first flagged ptx_render_nee.
	struct EnvTable {
		bool built = false, on_device = false;
		uint32_t w = 0, h = 0;
		std::vector<float> row_cdf, cell_cdf;   // [h], [h][w]
	} env_table;
	DevBuf d_env_row, d_env_cell;
	// The punctual lights of ptx_scene_set_punctual_lights, as stored, and their CDF; both empty: none. Guarded by lights_mu (and, on a scene
	// with a context, set under the context's mutex as well, so that no render is in flight). The device copies are made by the first
	// ptx_render_nee after a set.
	struct Punctual {
		bool on_device = false;
		std::vector<float> recs, cdf;   // [n][16], [n]
		std::vector<uint32_t> tree;     // [n_nodes][8] the light tree (build_punctual_tree); empty in CDF mode and without lights
	} punctual;
	uint32_t punctual_pick = PTX_PUNCTUAL_PICK_CDF;   // ptx_scene_set_punctual_pick; outlives the lights, guarded as they are
	DevBuf d_punctual, d_punctual_cdf, d_punctual_tree;
	// The motion table (ptx_scene_set_motion): begin transforms, current transforms, moved flags, in one buffer; dev_motion points into it
	// while the scene's motion moves a model, and is all nullptr otherwise. The begin camera travels in kernel arguments.
	DevBuf d_motion;
	DevMotion dev_motion{};
	DevBuf d_lens;   // the aperture table (kLensMaxBlades + 1 corners), allocated by upload_scene, refreshed in stream order by ptx_scene_set_camera
};

const ptx_scene::LightList* build_lights(ptx_scene* sc);   // ptx_api.cpp
// Whether a time-dependent state is in force (ptx_scene_set_motion with a model or the camera moving). The caller holds the context's mutex.
inline bool motion_active(const ptx_scene* sc) { return sc->host.motion.active(); }
// What the entry points that know no time answer while motion is active: PTX_ERR_UNSUPPORTED, before any device work
int refuse_motion(const char* who);   // ptx_api.cpp
const ptx_scene::EnvTable* build_env_table(ptx_scene* sc);   // ptx_api.cpp
// api_render.cpp: the scene's punctual lights as the kernels take them (records, CDF and, in tree mode, the tree), uploaded at the first
// call after a change; Pn stays empty without lights. The caller holds the context's mutex and has set the device.
int punctual_on_device_locked(ptx_scene* sc, NeePunctual& Pn);
// api_render.cpp: the light list as the kernels take it (and, in tree mode, the tree and the path words), built at the first request and
// uploaded at the first call after a change; Lt stays empty with an empty list. The caller holds the context's mutex and has set the device.
int lights_on_device_locked(ptx_scene* sc, NeeLights& Lt);
void srgb_thresholds(float thr[256]);                      // ptx_api.cpp
// api_batch.cpp: one decision on device buffers (adaptive.hip), its count read back: the stream is synchronised. The caller holds the
// context's mutex. select_ms: nullptr, or where the HIP-event time of the decision kernels is added.
int adaptive_decide_locked(ptx_ctx* c, uint32_t w, uint32_t h, const float4* d_a, const float4* d_b, float threshold, uint8_t* d_done, uint32_t* d_pixels, uint32_t& n_active,
                           double* select_ms);
// The same for a rank of a sharded call: the noisy bytes of its own pixels -> the registered exchange (c->mask_exchange; the stream is
// synchronised before the callback) -> the decision of the whole rectangle from the merged mask. d_pixels receives the rank's own active
// pixels, n_own their number, n_all the number of all active pixels of the rectangle: 8 bytes read back with one more synchronisation.
// mask_on_device: what the caller's mask buffer is; a host one is copied out of and back into the workspace. A callback that returns
// non-zero ends the decision with PTX_ERR_HIP and `exchange_failed` set.
int adaptive_decide_sharded_locked(ptx_ctx* c, uint32_t w, uint32_t h, const AdaptiveShard& shard, bool mask_on_device, const float4* d_a, const float4* d_b, float threshold,
                                   uint8_t* d_done, uint32_t* d_pixels, uint32_t& n_own, uint32_t& n_all, double* select_ms, bool& exchange_failed);

// A caller's buffer as the kernels take it. Device memory is used where it is. Host memory is staged at `off` in `buf` — copied in on
// the context's stream unless the buffer is output-only — and copy_back() queues the copy out; the entry point synchronises once, after
// its last copy_back. Several buffers staged in ONE DevBuf: ensure() the whole of it first (a growing ensure() frees what is staged).
struct Staged {
	void* host = nullptr;   // the caller's pointer where it is host memory
	void* d = nullptr;      // what the kernels take
	size_t bytes = 0;
	hipError_t bind(ptx_ctx* c, bool on_device, const void* p, size_t n_bytes, DevBuf& buf, size_t off = 0, bool copy_in = true) {
		d = const_cast<void*>(p);
		bytes = n_bytes;
		if (on_device) return hipSuccess;
		if (const hipError_t e = buf.ensure(off + n_bytes); e != hipSuccess) return e;
		host = d;
		d = (char*)buf.p + off;
		return copy_in ? hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
	}
	hipError_t copy_back(ptx_ctx* c, size_t n_bytes = SIZE_MAX) const {
		return host ? hipMemcpyAsync(host, d, std::min(n_bytes, bytes), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
	}
	template <class T> T* as() const { return (T*)d; }
};
constexpr bool kOutputOnly = false;   // Staged::bind's copy_in

// Bump carver of a workspace: take<T>(count) hands out consecutive arrays. On a null base it only measures, so the same carve run
// twice — on nullptr, then on the buffer — sizes the ensure() and lays the arrays out from one source.
struct Carver {
	char* base;
	size_t off = 0;
	explicit Carver(void* b) : base((char*)b) {}
	template <class T> T* take(size_t count) {
		T* const p = base ? (T*)(base + off) : nullptr;
		off += count * sizeof(T);
		return p;
	}
};

// the six ray pointers / six closest-hit pointers of an IntersectArgs: arrays `stride` entries apart from `base`
inline void ray_args(IntersectArgs& A, const float* base, size_t stride) {
	A.ox = base; A.oy = base + stride; A.oz = base + 2 * stride; A.dx = base + 3 * stride; A.dy = base + 4 * stride; A.dz = base + 5 * stride;
}
inline void hit_args(IntersectArgs& A, float* base, size_t stride) {
	A.distance = base; A.surface = (int32_t*)(base + stride); A.triangle = (int32_t*)(base + 2 * stride);
	A.b0 = base + 3 * stride; A.b1 = base + 4 * stride; A.b2 = base + 5 * stride;
}

// What every render entry point refuses in a cfg, decided before any device work; -> the rectangle. `who`: the entry point, for the
// message. check_bounces = false: ptx_render_aov, which ignores cfg->bounces.
inline int render_rect(const ptx_render_cfg* cfg, const char* who, bool check_bounces, uint32_t& x0, uint32_t& y0, uint32_t& w, uint32_t& h) {
	auto bad = [who](const char* m) { return set_err(PTX_ERR_INVALID, std::string(who) + ": " + m); };
	if (!cfg->W || !cfg->H) return bad("W and H must be > 0");   // bounces = 0 is legal: a black frame (renderer.cpp:438-439)
	x0 = cfg->x0; y0 = cfg->y0; w = cfg->w; h = cfg->h;
	if (w == 0 && h == 0) { x0 = 0; y0 = 0; w = cfg->W; h = cfg->H; }
	if (!w || !h || (uint64_t)x0 + w > cfg->W || (uint64_t)y0 + h > cfg->H) return bad("tile outside the image");
	if (check_bounces && cfg->bounces > 0xFFFFu) return bad("bounces > 65535");
	if (cfg->integrator > PTX_INTEGRATOR_WORKER) return bad("unknown integrator");
	if (cfg->shard_count > 1 && cfg->shard_index >= cfg->shard_count) return bad("shard_index >= shard_count");
	if ((uint64_t)w * h > 0x7FFFFFFFull) return bad("tile too large");
	return PTX_OK;
}

// samples of every pixel per launch: cfg->spp_per_pass, or by default what gives `default_samples` per pass; at most cfg->spp and at
// most `max_ids` samples in all. 0: one sample of every pixel is already too many for one pass
inline uint32_t pass_size(const ptx_render_cfg* cfg, uint64_t n_pixels, uint64_t default_samples, uint64_t max_ids) {
	uint32_t pass_spp = cfg->spp_per_pass ? cfg->spp_per_pass : (uint32_t)std::max<uint64_t>(1, default_samples / n_pixels);
	pass_spp = std::min(pass_spp, cfg->spp);
	while ((uint64_t)pass_spp * n_pixels > max_ids) pass_spp--;
	return pass_spp;
}

// An explicit device list of tile-local pixel indices for a pass to render in place of pixel_list()'s (ptx_render_adaptive's active list)
struct PixelSubset {
	const uint32_t* d_pixels;
	uint32_t n_pixels;
};

// The passes of one render call: the validated rectangle, the pixels (pixel_list() or a subset) and how the samples are cut into passes.
// Pass p is timed by events 2p and 2p + 1 of the context's pool when the caller asked for stats.
struct PassFrame {
	const ptx_render_cfg* cfg = nullptr;
	uint32_t x0 = 0, y0 = 0, w = 0, h = 0;
	uint64_t n_pixels = 0;
	const uint32_t* d_pixels = nullptr;
	uint32_t pass_spp = 0, n_pass = 0;   // n_pass == 0: nothing to render (spp == 0, or no tile of this shard meets the rectangle)

	// after render_rect: the pixels and the pass size (api_render.cpp). The caller holds the context's mutex.
	int plan(ptx_ctx* c, const ptx_scene* sc, const char* who, const PixelSubset* subset, uint64_t default_samples, uint64_t max_ids);
	uint64_t rect_pixels() const { return (uint64_t)w * h; }
	// RenderParams of pass p. shading = false leaves bounces and env zero (ptx_render_aov); `transparent` is the caller's to set.
	RenderParams params(uint32_t p, bool shading) const {
		RenderParams P{};
		P.W = cfg->W; P.H = cfg->H; P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
		P.n_pixels = (uint32_t)n_pixels;
		P.sample0 = cfg->sample0 + p * pass_spp;
		P.pass_spp = std::min(pass_spp, cfg->spp - p * pass_spp);
		P.n_paths = (uint64_t)P.pass_spp * n_pixels;
		P.seed_lo = cfg->seed_lo; P.seed_hi = cfg->seed_hi;
		if (shading) { P.bounces = cfg->bounces; memcpy(P.env, cfg->env, sizeof P.env); }
		P.integrator = cfg->integrator;
		P.pixels = d_pixels;
		return P;
	}
	// tops the context's event pool up to the 2 n events of n passes
	static int ensure_events(ptx_ctx* c, size_t n) {
		while (c->events.size() < 2 * n) {
			hipEvent_t ev;
			HIP_TRY(hipEventCreate(&ev));
			c->events.push_back(ev);
		}
		return PTX_OK;
	}
	// adds the elapsed times of passes 0 .. n - 1 to *ms; the stream is synchronised
	static int pass_ms(ptx_ctx* c, uint32_t n, double* ms) {
		for (uint32_t p = 0; p < n; p++) {
			float t = 0;
			HIP_TRY(hipEventElapsedTime(&t, c->events[2 * p], c->events[2 * p + 1]));
			*ms += t;
		}
		return PTX_OK;
	}
	// the ptx_render_stats (zeroed by the caller) of the finished call
	int stats(ptx_ctx* c, uint64_t rays, ptx_render_stats* st) const {
		st->rays = rays;
		st->samples = (uint64_t)cfg->spp * n_pixels;
		st->passes = n_pass;
		return pass_ms(c, n_pass, &st->kernel_ms);
	}
};

#pragma GCC visibility pop
