// C ABI of libptx_hip.so (declared in include/ptx.h). Host glue only: contexts, scene upload,
// pass scheduling, staging of host buffers. All arithmetic of the hot path lives in kernels.hip;
// there is no CPU fallback — GPU entry points fail with PTX_ERR_NO_DEVICE when no HIP device exists.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ptx.h"
#include "kernels.hpp"

using namespace ptx;

namespace {

thread_local std::string g_err;
int set_err(int code, const std::string& m) { g_err = m; return code; }
#define HIP_TRY(expr)                                                                                           \
	do {                                                                                                        \
		hipError_t e_ = (expr);                                                                                 \
		if (e_ != hipSuccess) return set_err(PTX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
	} while (0)

bool is_device_ptr(const void* p) {
	hipPointerAttribute_t a;
	hipError_t e = hipPointerGetAttributes(&a, p);
	if (e != hipSuccess) { (void)hipGetLastError(); return false; }
	return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

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

// image::write's quantiser for sRGB colour channels as a step function (kernels.hip: srgb8): thr[k] = the smallest float v in [0, 1]
// with byte(v) >= k, byte(v) = static_cast<uint8_t>(powf(v, 1 / 2.2F) * 255 + 0.5F) evaluated with this process's libm — the
// reference's own call (image.cpp:143-154). Floats in [0, 1] order like their bit patterns, so each threshold is a bisection over bits.
void srgb_thresholds(float thr[256]) {
	auto byte_of = [](uint32_t bits) {
		float v;
		memcpy(&v, &bits, 4);
		return (uint32_t)(uint8_t)(std::pow(v, 1 / 2.2F) * 255 + 0.5F);
	};
	thr[0] = 0.0f;
	for (uint32_t k = 1; k < 256; k++) {
		uint32_t lo = 0, hi = 0x3F800000u;   // byte(lo) = 0 < k <= 255 = byte(hi)
		while (hi - lo > 1) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (byte_of(mid) >= k) hi = mid; else lo = mid;
		}
		memcpy(&thr[k], &hi, 4);
	}
}

constexpr size_t kLdsBudget = 160 * 1024;
constexpr size_t kLeafOrderMaxBytes = (size_t)1 << 40;   // never reached: see decide_mode  // per-CU LDS on gfx950; one workgroup may take all of it

}  // namespace

struct ptx_ctx {
	std::atomic<int> refs{1};   // the caller's handle + one per scene created on it: a scene may outlive ptx_ctx_destroy
	int device = 0;
	hipStream_t stream = nullptr;
	int n_cu = 0;
	std::mutex mu;
	DevBuf queues, sample_rad, counters, spill, stage_a, stage_b, pixel_list, srgb_thr;
	DevBuf aov;   // workspace of ptx_render_aov: the streams, hits and per-sample records of one pass
	DevBuf denoise;   // workspace of ptx_denoise: four float4 state buffers per pixel, and the staging of host buffers
	// workspace of ptx_render_adaptive / ptx_adaptive_select: the decision's buffers (noisy bytes, block masks and offsets, tile counts and
	// offsets, the count word), the loop's `done` bytes and active list, and the staging of host buffers
	DevBuf adaptive, adaptive_state, adaptive_stage;
	hipEvent_t adaptive_ev[2] = {nullptr, nullptr};   // around the decision kernels (select_ms)
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
	DevBuf d_models, d_surfaces, d_materials, d_nodes, d_refs, d_tris, d_shade, d_tex, d_texels, d_lut, d_spaces, d_model_space, d_wf_order;
	DevBuf d_res_nodes, d_res_refs, d_res_tris, d_texels_f, d_hot;
	DevScene dev{};
	double lds_area_share = 0;     // share of the surfaces' box area (sum over surfaces) that belongs to LDS-resident surfaces: how much of what a ray can enter is served from LDS
	double wf_pairs_per_ray = 0;   // queue-based pipeline: pairs (ray, entered surface) per ray seen so far on this scene, 0 = not yet measured
	bool leaf_ordered = true; // global-memory copy of the triangle records: per leaf reference (true) or per triangle (false)
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
	} lights;
	std::mutex lights_mu;   // host-only scenes have no context whose mutex could guard the build
	DevBuf d_light_tris, d_light_cdf, d_light_geom, d_light_first;
};

namespace {

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// Residency plan -> kernel family. PTX_FORCE_GLOBAL / PTX_NO_HYBRID: measurement switches.
void decide_mode(ptx_scene* sc) {
	FlatScene& h = sc->host;
	// PTX_LDS_LEAF_ORDER=0/1: the resident copy all ref-indexed / leaf-ordered where it is cheap (the default); PTX_LDS_BUDGET: a smaller
	// budget for the residency plan, in bytes (measurement and tests; read once, here)
	if (sc->lds_leaf_order < 0) {
		const char* e = getenv("PTX_LDS_LEAF_ORDER");
		sc->lds_leaf_order = (e && e[0] == '0') ? 0 : 1;
		sc->lds_budget = kLdsBudget;
		if (const char* b = getenv("PTX_LDS_BUDGET")) sc->lds_budget = std::min<size_t>(kLdsBudget, (size_t)strtoull(b, nullptr, 10));
	}
	plan_residency(h, sc->lds_budget, sc->lds_leaf_order != 0);
	if (getenv("PTX_FORCE_GLOBAL") || h.n_resident == 0) sc->mode = MODE_GLOBAL;
	else if (h.n_resident == h.surfaces.size()) sc->mode = MODE_LDS;
	else sc->mode = getenv("PTX_NO_HYBRID") ? MODE_GLOBAL : MODE_HYBRID;
	if (sc->mode == MODE_GLOBAL) for (auto& sr : h.surfaces) sr.lds_root = 0xFFFFFFFFu;
	sc->lds_bytes = sc->mode == MODE_GLOBAL ? 0 : h.res_bytes;
	{
		double all = 0, res = 0;
		for (const SurfaceRec& sr : h.surfaces) {
			const double ex = sr.bmax[0] - sr.bmin[0], ey = sr.bmax[1] - sr.bmin[1], ez = sr.bmax[2] - sr.bmin[2];
			const double a = (ex > 0 && ey > 0 && ez > 0) ? 2 * (ex * ey + ey * ez + ex * ez) : 0;
			all += a;
			if (sr.lds_root != 0xFFFFFFFFu) res += a;
		}
		sc->lds_area_share = all > 0 ? res / all : 0;
	}
	// Leaf-ordered records duplicate a triangle once per leaf that references it (12x on deep SAH trees) and save a dependent fetch per
	// test. Measured up to 144 MB of records (the 262 k-triangle atrium, against 25 MB per triangle + references): the leaf order still
	// wins by 8 % — the dependent fetch costs more than the cache footprint (profiles/round2_ab_layout_blocksize.txt), so the threshold
	// is out of reach of any scene that fits the other limits. PTX_LEAF_ORDER=0/1 overrides (measurement).
	sc->leaf_ordered = h.kd_refs.size() * 48 <= kLeafOrderMaxBytes;
	if (const char* e = getenv("PTX_LEAF_ORDER")) sc->leaf_ordered = e[0] != '0';
}

int upload_scene(ptx_scene* sc) {
	ptx_ctx* c = sc->ctx;
	HIP_TRY(hipSetDevice(c->device));
	FlatScene& h = sc->host;
	auto up = [&](DevBuf& b, const void* src, size_t bytes, size_t padded) -> hipError_t {
		hipError_t e = b.ensure(std::max<size_t>(padded, 16));
		if (e != hipSuccess) return e;
		e = hipMemsetAsync(b.p, 0, std::max<size_t>(padded, 16), c->stream);
		if (e != hipSuccess) return e;
		return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
	};
	for (ModelRec& mr : h.models) interleave_boxes(mr);
	for (SurfaceRec& sr : h.surfaces) interleave_boxes(sr);
	HIP_TRY(up(sc->d_models, h.models.data(), h.models.size() * sizeof(ModelRec), h.models.size() * sizeof(ModelRec)));
	HIP_TRY(up(sc->d_materials, h.materials.data(), h.materials.size() * sizeof(MaterialRec), h.materials.size() * sizeof(MaterialRec)));
	HIP_TRY(up(sc->d_refs, h.kd_refs.data(), h.kd_refs.size() * 4, pad16(h.kd_refs.size() * 4)));
	HIP_TRY(up(sc->d_tris, h.hitrec.data(), h.hitrec.size() * sizeof(HitRec), h.hitrec.size() * sizeof(HitRec)));
	decide_mode(sc);   // sets SurfaceRec::lds_root: before the surface table goes up
	{
		// Hot hit records: what LDS is left beside the resident geometry takes the hit records (144 B) of the LARGEST triangles — where most
		// hits land (Cornell: walls, boxes, light) — so that shading them costs nine LDS reads instead of a round of nine global gathers
		// (9.8 % of the headline kernel's time, profiles/round3_clk_fused.txt). A triangle's slot travels in the top byte of the
		// triangle word of its traversal records (id | slot << 24; 0xFF = not hot), which needs ids below 2^24. PTX_NO_HOT_HITREC: measurement.
		const size_t n_tri = h.hitrec.size();
		const bool packed = n_tri < ((size_t)1 << 24);
		std::vector<uint8_t> slot_of(n_tri, 0xFF);
		h.hot_hitrec.clear();
		if (packed && sc->mode != MODE_GLOBAL && !getenv("PTX_NO_HOT_HITREC")) {
			const size_t left = kLdsBudget > sc->lds_bytes ? kLdsBudget - sc->lds_bytes : 0;
			const size_t n_hot = std::min<size_t>({(size_t)255, left / sizeof(HitRec), n_tri});
			if (n_hot) {
				std::vector<float> area(n_tri, 0.f);
				for (size_t si = 0; si < h.surfaces.size(); si++) {
					const int32_t* rg = &h.surf_range[8 * si];
					const ModelRec& mr = h.models[h.surfaces[si].model];
					double sc2 = 0;   // mean squared length of the basis columns: local -> world area scale (ranking only)
					for (int k = 0; k < 9; k++) sc2 += (double)mr.basis[k] * mr.basis[k];
					sc2 /= 3.0;
					for (int32_t t = rg[2]; t < rg[2] + rg[3]; t++) {
						const HitRec& r = h.hitrec[(size_t)t];
						const double e1[3] = {(double)r.b[0] - r.a[0], (double)r.b[1] - r.a[1], (double)r.b[2] - r.a[2]}, e2[3] = {(double)r.c[0] - r.a[0], (double)r.c[1] - r.a[1], (double)r.c[2] - r.a[2]};
						const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
						area[(size_t)t] = (float)(0.5 * std::sqrt(cx * cx + cy * cy + cz * cz) * sc2);
					}
				}
				std::vector<uint32_t> idx(n_tri);
				for (size_t i = 0; i < n_tri; i++) idx[i] = (uint32_t)i;
				std::partial_sort(idx.begin(), idx.begin() + (std::ptrdiff_t)n_hot, idx.end(), [&](uint32_t a, uint32_t b) { return area[a] != area[b] ? area[a] > area[b] : a < b; });
				for (size_t k = 0; k < n_hot; k++) { slot_of[idx[k]] = (uint8_t)k; h.hot_hitrec.push_back(h.hitrec[idx[k]]); }
				sc->lds_bytes += n_hot * sizeof(HitRec);
			}
		}
		auto pack = [&](std::vector<TriIsect>& recs) {
			for (TriIsect& r : recs) {
				uint32_t w; memcpy(&w, &r.p0, 4);
				const uint32_t id = packed ? (w & 0x00FFFFFFu) : w;
				w = packed ? (id | ((uint32_t)slot_of[id] << 24)) : id;
				memcpy(&r.p0, &w, 4);
			}
		};
		pack(h.tri_isect); pack(h.res_tris);
		sc->dev.tri_id_mask = packed ? 0x00FFFFFFu : 0xFFFFFFFFu;
		sc->dev.n_hot = (uint32_t)h.hot_hitrec.size();
	}
	HIP_TRY(up(sc->d_surfaces, h.surfaces.data(), h.surfaces.size() * sizeof(SurfaceRec), h.surfaces.size() * sizeof(SurfaceRec)));
	// KD nodes and the global-memory triangle records share ONE allocation: the queue-based traverse kernel addresses both as
	// `base + 32-bit offset` (wavefront.hip). + 16: the child-pair fetch of the last branch may read one node past the end.
	const size_t nodes_bytes = (pad16(h.kd_nodes.size() * 8) + 16 + 255) & ~(size_t)255;
	size_t isect_bytes = 0;
	std::vector<TriIsect> leaf;
	if (sc->mode != MODE_LDS) {
		if (sc->leaf_ordered) {
			// surfaces that stay in L2/HBM: one record per leaf reference, in leaf order, so that a leaf's triangles are one
			// contiguous run and the reference -> record indirection is gone (Geom::leaf_ordered)
			leaf.resize(h.kd_refs.size());
			for (size_t r = 0; r < leaf.size(); r++) leaf[r] = h.tri_isect[h.kd_refs[r]];
			isect_bytes = leaf.size() * 48;
		} else {
			// one record per TRIANGLE, reached through the leaf references: an extra dependent fetch per test, but a working set
			// (nodes + refs + records) several times smaller when leaves share many triangles
			isect_bytes = h.tri_isect.size() * 48;
		}
	}
	const size_t isect_pad = (std::max<size_t>(isect_bytes, 16) + 255) & ~(size_t)255;
	const size_t geom_total = nodes_bytes + isect_pad;
	HIP_TRY(sc->d_nodes.ensure(geom_total));
	HIP_TRY(hipMemsetAsync(sc->d_nodes.p, 0, geom_total, c->stream));
	if (!h.kd_nodes.empty()) HIP_TRY(hipMemcpyAsync(sc->d_nodes.p, h.kd_nodes.data(), h.kd_nodes.size() * 8, hipMemcpyHostToDevice, c->stream));
	if (isect_bytes)
		HIP_TRY(hipMemcpyAsync((char*)sc->d_nodes.p + nodes_bytes, sc->leaf_ordered ? (const void*)leaf.data() : (const void*)h.tri_isect.data(), isect_bytes, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));   // `leaf` is a local
	std::vector<TriIsect>().swap(leaf);
	if (sc->mode != MODE_GLOBAL) {
		HIP_TRY(up(sc->d_res_nodes, h.res_nodes.data(), h.res_nodes.size() * 8, pad16(h.res_nodes.size() * 8)));
		HIP_TRY(up(sc->d_res_refs, h.res_refs.data(), h.res_refs.size() * 4, pad16(h.res_refs.size() * 4)));
		HIP_TRY(up(sc->d_res_tris, h.res_tris.data(), h.res_tris.size() * 48, h.res_tris.size() * 48));
		HIP_TRY(up(sc->d_hot, h.hot_hitrec.data(), h.hot_hitrec.size() * sizeof(HitRec), h.hot_hitrec.size() * sizeof(HitRec)));
	}
	HIP_TRY(up(sc->d_shade, h.shade.data(), h.shade.size() * sizeof(ShadeRec), h.shade.size() * sizeof(ShadeRec)));
	HIP_TRY(up(sc->d_tex, h.textures.data(), h.textures.size() * sizeof(TexRec), h.textures.size() * sizeof(TexRec)));
	HIP_TRY(up(sc->d_texels, h.texels.data(), h.texels.size(), pad16(h.texels.size())));
	HIP_TRY(up(sc->d_texels_f, h.texels_f.data(), h.texels_f.size() * 4, pad16(h.texels_f.size() * 4)));
	{   // image::read: value = byte / 255.0F; sRGB colour channels: math::pow(value, 2.2F) (image.cpp:135-138) — same libm call, once per byte value
		float lut[256];
		for (int b = 0; b < 256; b++) lut[b] = std::pow(b / 255.0F, 2.2F);
		HIP_TRY(up(sc->d_lut, lut, sizeof lut, sizeof lut));
	}
	HIP_TRY(up(sc->d_spaces, h.spaces.data(), h.spaces.size() * sizeof(SpaceRec), h.spaces.size() * sizeof(SpaceRec)));
	HIP_TRY(up(sc->d_model_space, h.model_space.data(), h.model_space.size() * 4, h.model_space.size() * 4));
	{
		// The order in which the queue-based traverse kernel starts the surfaces' queues. A render's steps: largest tree first, so that
		// a launch ends on the queues of the short walks and the few long walks (hundreds of dependent fetches in the big trees) start
		// early — atrium 1080p 446 -> 471 Msamples/s, 4K / 16 bounces 394 -> 418, jack-of-blades 2229 -> 2326; smallest first: no change
		// (profiles/round3_surface_order.txt). ptx_intersect_batch's launches keep the surface order: on its 5-8 M-ray slices the sorted
		// order was 10 % slower on bounce rays (2 % faster on camera rays). Second half of the table: the batch order.
		// PTX_WF_ORDER / PTX_WF_ORDER_BATCH = 0 surface order, 1 largest tree first, 2 smallest first (measurement).
		const size_t ns = h.surfaces.size();
		std::vector<uint32_t> order(2 * ns);
		auto fill = [&](uint32_t* o, int om) {
			for (size_t i = 0; i < ns; i++) o[i] = (uint32_t)i;
			if (om != 0) std::stable_sort(o, o + ns, [&](uint32_t a, uint32_t b) {
				const int32_t na = h.surf_range[8 * a + 5], nb = h.surf_range[8 * b + 5];   // KD nodes of the surface
				return om == 2 ? na < nb : na > nb;
			});
		};
		const char *oe = getenv("PTX_WF_ORDER"), *ob = getenv("PTX_WF_ORDER_BATCH");
		fill(order.data(), oe ? atoi(oe) : 1);
		fill(order.data() + ns, ob ? atoi(ob) : 0);
		HIP_TRY(up(sc->d_wf_order, order.data(), order.size() * 4, order.size() * 4));
	}
	HIP_TRY(hipStreamSynchronize(c->stream));
	DevScene& d = sc->dev;
	d.models = (const ModelRec*)sc->d_models.p;
	d.surfaces = (const SurfaceRec*)sc->d_surfaces.p;
	d.materials = (const MaterialRec*)sc->d_materials.p;
	d.nodes = (const uint2*)sc->d_nodes.p;
	d.refs = (const uint32_t*)sc->d_refs.p;
	d.tris = (const float4*)sc->d_tris.p;
	d.tri_isect = isect_bytes ? (const float4*)((const char*)sc->d_nodes.p + nodes_bytes) : nullptr;
	d.geom_bytes = (uint64_t)geom_total;
	d.res_nodes = (const uint2*)sc->d_res_nodes.p;
	d.res_refs = (const uint32_t*)sc->d_res_refs.p;
	d.res_tris = (const float4*)sc->d_res_tris.p;
	d.hot_hitrec = (const float4*)sc->d_hot.p;
	d.hot_lds = nullptr;
	d.n_res_nodes = (uint32_t)h.res_nodes.size();
	d.n_res_refs = (uint32_t)h.res_refs.size();
	d.n_res_tris = (uint32_t)h.res_tris.size();
	d.shade = (const ShadeRec*)sc->d_shade.p;
	d.spaces = (const SpaceRec*)sc->d_spaces.p;
	d.tex = (const TexRec*)sc->d_tex.p;
	d.texels = (const uint8_t*)sc->d_texels.p;
	d.texels_f = (const float*)sc->d_texels_f.p;
	d.srgb_lut = (const float*)sc->d_lut.p;
	d.glb_leaf_ordered = sc->leaf_ordered ? 1u : 0u;
	d.any_texture = (h.any_texture || h.env_tex >= 0) ? 1u : 0u;   // the TEX kernels also carry the environment lookup
	d.env_tex = h.env_tex;
	d.model_space = (const uint32_t*)sc->d_model_space.p;
	d.wf_order = (const uint32_t*)sc->d_wf_order.p;
	d.n_spaces = (uint32_t)h.spaces.size();
	d.n_surfaces = (uint32_t)h.surfaces.size();
	d.any_alpha = h.any_alpha ? 1u : 0u;
	d.n_models = (int32_t)h.models.size();
	d.n_nodes = (uint32_t)h.kd_nodes.size();
	d.n_refs = (uint32_t)h.kd_refs.size();
	d.n_tris = (uint32_t)h.tris.size();
	d.cam = h.camera;
	d.sun = h.sun;
	return PTX_OK;
}

void release_scene_buffers(ptx_scene* sc) {
	for (DevBuf* b : {&sc->d_models, &sc->d_surfaces, &sc->d_materials, &sc->d_nodes, &sc->d_refs, &sc->d_tris, &sc->d_shade, &sc->d_tex,
	                  &sc->d_texels, &sc->d_texels_f, &sc->d_lut, &sc->d_spaces, &sc->d_model_space, &sc->d_wf_order, &sc->d_res_nodes, &sc->d_res_refs, &sc->d_res_tris, &sc->d_hot,
	                  &sc->d_light_tris, &sc->d_light_cdf, &sc->d_light_geom, &sc->d_light_first})
		b->release();
	sc->lights.on_device = false;
}

int finish_scene(ptx_ctx* ctx, ptx_scene* sc, ptx_scene** out) {
	sc->ctx = ctx;
	if (ctx) {
		std::lock_guard<std::mutex> lk(ctx->mu);
		int rc = upload_scene(sc);
		if (rc != PTX_OK) { release_scene_buffers(sc); delete sc; return rc; }
		ctx->refs.fetch_add(1);
	} else {
		decide_mode(sc);
	}
	*out = sc;
	return PTX_OK;
}

}  // namespace

extern "C" {

const char* ptx_last_error(void) { return g_err.c_str(); }
const char* ptx_version(void) { return "ptx_hip 0.1 (gfx950)"; }

int ptx_ctx_create(int device, ptx_ctx** out) {
	if (!out) return set_err(PTX_ERR_INVALID, "ptx_ctx_create: out is NULL");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		(void)hipGetLastError();
		return set_err(PTX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
	}
	if (device < 0 || device >= n) return set_err(PTX_ERR_INVALID, "device ordinal out of range");
	HIP_TRY(hipSetDevice(device));
	ptx_ctx* c = new ptx_ctx;
	c->device = device;
	hipDeviceProp_t prop;
	e = hipGetDeviceProperties(&prop, device);
	if (e != hipSuccess) { delete c; return set_err(PTX_ERR_HIP, hipGetErrorString(e)); }
	c->n_cu = prop.multiProcessorCount;
	e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
	if (e != hipSuccess) { delete c; return set_err(PTX_ERR_HIP, hipGetErrorString(e)); }
	*out = c;
	return PTX_OK;
}

static void ctx_release(ptx_ctx* c) {
	if (c->refs.fetch_sub(1) != 1) return;   // scenes still alive: the last one frees the context
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
	for (hipEvent_t ev : c->step_events) (void)hipEventDestroy(ev);
	c->queues.release(); c->spill.release(); c->sample_rad.release(); c->counters.release(); c->stage_a.release(); c->stage_b.release(); c->pixel_list.release(); c->srgb_thr.release(); c->aov.release(); c->denoise.release();
	c->adaptive.release(); c->adaptive_state.release(); c->adaptive_stage.release();
	for (hipEvent_t ev : c->adaptive_ev) if (ev) (void)hipEventDestroy(ev);
	ptx_ctx::WfSet& w = c->wf;
	for (DevBuf* b : {&w.qent, &w.pair_hit, &w.seg, &w.first, &w.mask, &w.ctl, &w.spill, &w.stream_buf, &w.flow}) b->release();
	if (w.flow_host) { (void)hipHostFree(w.flow_host); w.flow_host = nullptr; }
	(void)hipStreamDestroy(c->stream);
	delete c;
}
void ptx_ctx_destroy(ptx_ctx* c) {
	if (c) ctx_release(c);
}

void* ptx_ctx_stream(ptx_ctx* c) { return c ? (void*)c->stream : nullptr; }

int ptx_ctx_synchronize(ptx_ctx* c) {
	if (!c) return set_err(PTX_ERR_INVALID, "ctx is NULL");
	HIP_TRY(hipStreamSynchronize(c->stream));
	return PTX_OK;
}

int ptx_ctx_set_timing(ptx_ctx* c, int on) {
	if (!c) return set_err(PTX_ERR_INVALID, "ctx is NULL");
	std::lock_guard<std::mutex> lk(c->mu);
	c->timing_on = on != 0;
	return PTX_OK;
}

int ptx_ctx_get_timing(ptx_ctx* c, ptx_kernel_timing* out) {
	if (!c || !out) return set_err(PTX_ERR_INVALID, "NULL argument");
	std::lock_guard<std::mutex> lk(c->mu);
	*out = c->timing;
	return PTX_OK;
}

int ptx_scene_load_gltf(ptx_ctx* ctx, const char* path, const ptx_load_opts* opts, ptx_scene** out) {
	if (!path || !out) return set_err(PTX_ERR_INVALID, "ptx_scene_load_gltf: NULL argument");
	ptx_scene* sc = new ptx_scene;
	try {
		WorkFilter wf;
		if (opts && opts->filter_primitives) {
			wf.filter = true;
			for (uint32_t k = 0; k < opts->n_work; k++) {
				const ptx_work_item& it = opts->work[k];
				wf.work.emplace_back(it.mesh_name ? it.mesh_name : "", std::vector<int32_t>(it.primitives, it.primitives + it.n_primitives));
			}
		}
		load_gltf(path, opts ? opts->camera_index : 0u, opts ? opts->sun_light_index : 0u, wf, sc->host);
	} catch (const Error& e) {
		delete sc;
		return set_err(e.code, e.msg);
	} catch (const std::exception& e) {
		delete sc;
		return set_err(PTX_ERR_PARSE, e.what());
	}
	return finish_scene(ctx, sc, out);
}

int ptx_worker_event_load(ptx_ctx* ctx, const char* event_json_path, const char* local_scene_root, ptx_scene** scene, ptx_render_cfg* cfg,
                          ptx_worker_event* info) {
	if (!event_json_path || !local_scene_root || !scene || !cfg) return set_err(PTX_ERR_INVALID, "ptx_worker_event_load: NULL argument");
	ptx_scene* sc = new ptx_scene;
	try {
		WorkerEvent ev;
		parse_worker_event(event_json_path, ev);
		if (ev.samples < 0 || ev.bounces <= 0 || !(ev.X >= 1) || !(ev.Y >= 1)) throw Error{PTX_ERR_INVALID, "worker event: samples / bounces / X / Y out of range"};
		std::string root = local_scene_root;
		if (!root.empty() && root.back() != '/') root += '/';
		load_gltf(root + "scene.gltf", 0u, 0u, ev.work, sc->host);   // worker::download_gltf_file: scene_root + "scene.gltf" (worker.cpp:108-112)
		*cfg = ptx_render_cfg{};
		cfg->W = (uint32_t)ev.X; cfg->H = (uint32_t)ev.Y;            // worker.cpp:36-38
		cfg->spp = (uint32_t)ev.samples; cfg->bounces = (uint32_t)ev.bounces;
		cfg->env[0] = cfg->env[1] = cfg->env[2] = 1.0f;
		cfg->seed_lo = 0x5EEDu;
		cfg->integrator = PTX_INTEGRATOR_WORKER;                      // what processors::worker::run renders with
		if (info) {
			*info = ptx_worker_event{};
			info->num_workers = ev.num_workers;
			info->n_work_meshes = (uint32_t)ev.work.work.size();
			snprintf(info->worker_id, sizeof info->worker_id, "%s", ev.worker_id.c_str());
			snprintf(info->scene_root, sizeof info->scene_root, "%s", ev.scene_root.c_str());
			snprintf(info->scene_bucket, sizeof info->scene_bucket, "%s", ev.scene_bucket.c_str());
		}
	} catch (const Error& e) {
		delete sc;
		return set_err(e.code, e.msg);
	} catch (const std::exception& e) {
		delete sc;
		return set_err(PTX_ERR_PARSE, e.what());
	}
	return finish_scene(ctx, sc, scene);
}

int ptx_scene_set_environment(ptx_scene* sc, const char* png_path, int srgb) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_scene_set_environment: scene is NULL");
	// the file is read before the lock is taken; the scene's host arrays are only touched under it (a render may be in flight on
	// another thread: ptx_render holds the same mutex for its whole call)
	FlatScene img;   // the decoded file: one TexRec + its texels (8-bit or, for a Radiance .hdr, float)
	TexRec rec{};
	try {
		if (png_path) rec = load_texture(img, png_path, srgb != 0);   // PNG, JPEG or .hdr, by content
	} catch (const Error& e) {
		return set_err(e.code, e.msg);
	} catch (const std::exception& e) {
		return set_err(PTX_ERR_PARSE, e.what());
	}
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);
	FlatScene& h = sc->host;
	if (h.env_tex >= 0) {   // the previous map is always the last texture (appended below): drop it instead of letting them pile up
		const TexRec old = h.textures[(size_t)h.env_tex];
		if (old.c_srgb & kTexFloat) h.texels_f.resize(old.offset); else h.texels.resize(old.offset);
		h.textures.pop_back();
		h.texture_paths.pop_back();
		h.env_tex = -1;
	}
	if (png_path) {
		if (rec.c_srgb & kTexFloat) { rec.offset = (uint32_t)h.texels_f.size(); h.texels_f.insert(h.texels_f.end(), img.texels_f.begin(), img.texels_f.end()); }
		else { rec.offset = (uint32_t)h.texels.size(); h.texels.insert(h.texels.end(), img.texels.begin(), img.texels.end()); }
		h.textures.push_back(rec);
		h.texture_paths.push_back(png_path);
		h.env_tex = (int32_t)h.textures.size() - 1;
	}
	if (sc->ctx) return upload_scene(sc);   // textures changed: the whole (small) scene goes up again
	return PTX_OK;
}

int ptx_scene_from_arrays(ptx_ctx* ctx, const ptx_scene_desc* d, ptx_scene** out) {
	if (!d || !out) return set_err(PTX_ERR_INVALID, "ptx_scene_from_arrays: NULL argument");
	if (!d->camera || (d->n_models && (!d->model_xform || !d->model_surf)) ||
	    (d->n_surfaces && (!d->surf_range || !d->vertices || !d->triangles || !d->materials)))
		return set_err(PTX_ERR_INVALID, "ptx_scene_from_arrays: missing array");
	ptx_scene* sc = new ptx_scene;
	FlatScene& h = sc->host;
	try {
		h.model_xform.assign(d->model_xform, d->model_xform + 12 * (size_t)d->n_models);
		h.model_surf.assign(d->model_surf, d->model_surf + 2 * (size_t)d->n_models);
		size_t nv = 0, nt = 0;
		for (uint32_t s = 0; s < d->n_surfaces; s++) {
			const int32_t* r = d->surf_range + 4 * (size_t)s;
			if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0) throw Error{PTX_ERR_INVALID, "negative surface range"};
			int32_t rg[8] = {r[0], r[1], r[2], r[3], 0, 0, 0, 0};
			h.surf_range.insert(h.surf_range.end(), rg, rg + 8);
			nv = std::max(nv, (size_t)r[0] + r[1]);
			nt = std::max(nt, (size_t)r[2] + r[3]);
		}
		h.vertices.assign(d->vertices, d->vertices + 11 * nv);
		h.triangles.assign(d->triangles, d->triangles + 3 * nt);
		for (uint32_t s = 0; s < d->n_surfaces; s++) {
			const int32_t* r = &h.surf_range[8 * (size_t)s];
			for (int32_t t = 0; t < 3 * r[3]; t++)
				if (h.triangles[3 * (size_t)r[2] + t] >= (uint32_t)r[1]) throw Error{PTX_ERR_INVALID, "vertex index out of range"};
		}
		for (uint32_t m = 0; m < d->n_models; m++) {
			int32_t f = h.model_surf[2 * m], n = h.model_surf[2 * m + 1];
			if (f < 0 || n < 0 || (uint32_t)(f + n) > d->n_surfaces) throw Error{PTX_ERR_INVALID, "model surface range out of bounds"};
			if (f != (m ? h.model_surf[2 * m - 2] + h.model_surf[2 * m - 1] : 0)) throw Error{PTX_ERR_INVALID, "model surface ranges must be consecutive, in model order"};
			h.model_names.push_back("model" + std::to_string(m));
		}
		h.materials_raw.assign(d->materials, d->materials + 11 * (size_t)d->n_surfaces);
		h.material_tex.assign(7 * (size_t)d->n_surfaces, 0);
		finalize_scene(h, d->camera, d->sun);
	} catch (const Error& e) {
		delete sc;
		return set_err(e.code, e.msg);
	} catch (const std::exception& e) {
		delete sc;
		return set_err(PTX_ERR_INVALID, e.what());
	}
	return finish_scene(ctx, sc, out);
}

void ptx_scene_destroy(ptx_scene* sc) {
	if (!sc) return;
	if (sc->ctx) {
		std::lock_guard<std::mutex> lk(sc->ctx->mu);
		(void)hipSetDevice(sc->ctx->device);
		(void)hipStreamSynchronize(sc->ctx->stream);
		release_scene_buffers(sc);
	}
	ptx_ctx* c = sc->ctx;
	delete sc;
	if (c) ctx_release(c);
}

int ptx_scene_get_info(const ptx_scene* sc, ptx_scene_info* info) {
	if (!sc || !info) return set_err(PTX_ERR_INVALID, "NULL argument");
	const FlatScene& h = sc->host;
	info->n_models = (uint32_t)h.models.size();
	info->n_surfaces = (uint32_t)h.surfaces.size();
	info->n_vertices = (uint32_t)(h.vertices.size() / 11);
	info->n_triangles = (uint32_t)h.tris.size();
	info->n_kd_nodes = (uint32_t)h.kd_nodes.size();
	info->n_kd_refs = (uint32_t)h.kd_refs.size();
	info->kd_max_depth = h.kd_max_depth;
	info->has_sun = h.sun.present;
	info->geometry_bytes = (uint32_t)sc->host.geometry_bytes();
	info->lds_resident = (uint32_t)sc->mode;
	info->n_textures = (uint32_t)h.textures.size();
	return PTX_OK;
}

namespace {

// The emissive triangles ptx_render_nee samples (include/ptx.h: the listing rules). World corners, areas and normals in float64 in the
// written order, stored as float32.
const ptx_scene::LightList* build_lights(ptx_scene* sc) {
	std::lock_guard<std::mutex> lk(sc->lights_mu);
	ptx_scene::LightList& ll = sc->lights;
	if (ll.built) return &ll;
	const FlatScene& h = sc->host;
	const size_t n_surf = h.surfaces.size();
	ll.surf_first.assign(n_surf, -1);
	std::vector<double> cum;
	double total = 0;
	for (size_t s = 0; s < n_surf; s++) {
		const MaterialRec& m = h.materials[s];
		if (!(m.emissive[0] > 0 || m.emissive[1] > 0 || m.emissive[2] > 0)) continue;
		if (m.tex[2] >= 0 || !(m.opacity == 1.0f || std::fabs(m.opacity - 1.0f) < 0.0001f) || m.shadow_catcher) continue;   // can pass a sample through
		const float* X = h.model_xform.data() + 12 * (size_t)h.surfaces[s].model;
		const int32_t* rg = h.surf_range.data() + 8 * s;
		for (int32_t t = 0; t < rg[3]; t++) {
			double c[3][3];
			for (int k = 0; k < 3; k++) {
				const float* v = h.vertices.data() + 11 * (size_t)(rg[0] + (int32_t)h.triangles[3 * (size_t)(rg[2] + t) + k]);
				for (int a = 0; a < 3; a++) c[k][a] = ((double)X[3 + a] * (double)v[0] + (double)X[6 + a] * (double)v[1]) + (double)X[9 + a] * (double)v[2] + (double)X[a];
			}
			const double e1[3] = {c[1][0] - c[0][0], c[1][1] - c[0][1], c[1][2] - c[0][2]}, e2[3] = {c[2][0] - c[0][0], c[2][1] - c[0][1], c[2][2] - c[0][2]};
			const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
			const double len = std::sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
			const double area = 0.5 * len;
			if (!(area > 0)) continue;
			if (ll.surf_first[s] < 0) ll.surf_first[s] = (int32_t)(ll.tris.size() / 2);
			ll.tris.push_back((uint32_t)s); ll.tris.push_back((uint32_t)t);
			for (int a = 0; a < 3; a++) ll.geom.push_back((float)(cr[a] / len));
			ll.geom.push_back((float)area);
			total += area;
			cum.push_back(total);
		}
	}
	for (double v : cum) ll.cdf.push_back((float)(v / total));
	if (!ll.cdf.empty()) ll.cdf.back() = 1.0f;
	ll.area = (float)total;
	ll.built = true;
	return &ll;
}

}  // namespace

int64_t ptx_scene_get_array(const ptx_scene* sc, ptx_array which, void* dst, size_t dst_bytes) {
	if (!sc) { set_err(PTX_ERR_INVALID, "scene is NULL"); return -1; }
	const FlatScene& h = sc->host;
	const void* src = nullptr;
	size_t bytes = 0, elem = 4;
	std::vector<float> tmp;
	std::string names;
	switch (which) {
	case PTX_ARR_MODEL_XFORM: src = h.model_xform.data(); bytes = h.model_xform.size() * 4; break;
	case PTX_ARR_MODEL_AABB:
		for (auto& m : h.models) { tmp.insert(tmp.end(), m.bmin, m.bmin + 3); tmp.insert(tmp.end(), m.bmax, m.bmax + 3); }
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_MODEL_SURF: src = h.model_surf.data(); bytes = h.model_surf.size() * 4; break;
	case PTX_ARR_SURF_RANGE: src = h.surf_range.data(); bytes = h.surf_range.size() * 4; break;
	case PTX_ARR_MESH_AABB:
		for (auto& s : h.surfaces) { tmp.insert(tmp.end(), s.bmin, s.bmin + 3); tmp.insert(tmp.end(), s.bmax, s.bmax + 3); }
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_VERTICES: src = h.vertices.data(); bytes = h.vertices.size() * 4; break;
	case PTX_ARR_TRIANGLES: src = h.triangles.data(); bytes = h.triangles.size() * 4; break;
	case PTX_ARR_MATERIALS: src = h.materials_raw.data(); bytes = h.materials_raw.size() * 4; break;
	case PTX_ARR_KD_NODES: src = h.kd_nodes.data(); bytes = h.kd_nodes.size() * 8; break;
	case PTX_ARR_KD_REFS: src = h.kd_refs.data(); bytes = h.kd_refs.size() * 4; break;
	case PTX_ARR_CAMERA:
		tmp.assign(h.camera.origin, h.camera.origin + 3); tmp.insert(tmp.end(), h.camera.basis, h.camera.basis + 9);
		tmp.push_back(h.camera.fov); tmp.push_back(h.camera.tan_half_fov);
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_SUN:
		if (h.sun.present) { tmp.assign(h.sun.basis, h.sun.basis + 9); tmp.insert(tmp.end(), h.sun.energy, h.sun.energy + 3); tmp.push_back(h.sun.angular_radius); }
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_MODEL_NAMES:
		for (auto& n : h.model_names) names += n + "\n";
		src = names.data(); bytes = names.size(); elem = 1; break;
	case PTX_ARR_TEXTURES: src = h.textures.data(); bytes = h.textures.size() * sizeof(TexRec); break;
	case PTX_ARR_TEXELS: src = h.texels.data(); bytes = h.texels.size(); elem = 1; break;
	case PTX_ARR_SURF_TEX: src = h.surf_tex.data(); bytes = h.surf_tex.size() * 4; break;
	case PTX_ARR_TEXELS_F32: src = h.texels_f.data(); bytes = h.texels_f.size() * 4; break;
	case PTX_ARR_LIGHT_TRIS: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.tris.data(); bytes = ll.tris.size() * 4; break; }
	case PTX_ARR_LIGHT_CDF: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.cdf.data(); bytes = ll.cdf.size() * 4; break; }
	case PTX_ARR_LIGHT_GEOM: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.geom.data(); bytes = ll.geom.size() * 4; break; }
	case PTX_ARR_TRI_ISECT: src = h.tri_isect.data(); bytes = h.tri_isect.size() * sizeof(TriIsect); break;
	case PTX_ARR_RES_NODES: src = h.res_nodes.data(); bytes = h.res_nodes.size() * 8; break;
	case PTX_ARR_RES_REFS: src = h.res_refs.data(); bytes = h.res_refs.size() * 4; break;
	case PTX_ARR_RES_TRIS: src = h.res_tris.data(); bytes = h.res_tris.size() * sizeof(TriIsect); break;
	case PTX_ARR_LDS_ROOT:
		for (auto& s : h.surfaces) { float f; memcpy(&f, &s.lds_root, 4); tmp.push_back(f); }
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_RES_PLAN: {
		const uint32_t w[4] = {(uint32_t)h.res_bytes, h.n_resident, (uint32_t)sc->lds_bytes, (uint32_t)h.hot_hitrec.size()};
		tmp.resize(4); memcpy(tmp.data(), w, 16);
		src = tmp.data(); bytes = 16; break;
	}
	default: set_err(PTX_ERR_INVALID, "unknown array id"); return -1;
	}
	if (dst) {
		if (dst_bytes < bytes) { set_err(PTX_ERR_INVALID, "destination too small"); return -1; }
		if (bytes) memcpy(dst, src, bytes);
	}
	return (int64_t)(bytes / elem);
}

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

// samples of every pixel per launch: enough paths to fill the chip many times over, bounded workspace; 0: one sample of every pixel
// is already too many paths for one pass
uint32_t pass_size(const ptx_render_cfg* cfg, uint64_t n_pixels) {
	uint32_t pass_spp = cfg->spp_per_pass;
	if (pass_spp == 0) {
		const uint64_t target_paths = 128ull << 20;   // 64 spp of a 1080p frame: 2 GB of per-sample radiance; fewer, longer launches (measured: 8 -> 64 spp per launch = +11 %)
		pass_spp = (uint32_t)std::max<uint64_t>(1, target_paths / n_pixels);
	}
	pass_spp = std::min(pass_spp, cfg->spp);
	while ((uint64_t)pass_spp * n_pixels > 0xFFFFFFFFull) pass_spp--;  // path ids are 32-bit
	return pass_spp;
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
int render_stats(ptx_ctx* c, uint64_t samples, uint32_t n_pass, bool wavefront, const WfPlan& plan, const WfClock& clk, unsigned long long wf_rays,
                 ptx_render_stats* stats) {
	unsigned long long rays = 0;
	HIP_TRY(hipMemcpy(&rays, (char*)c->counters.p + 16, 8, hipMemcpyDeviceToHost));
	stats->rays = rays + wf_rays;
	stats->samples = samples;
	stats->passes = n_pass;
	double ms = 0;
	for (uint32_t p = 0; p < n_pass; p++) {
		float t = 0;
		HIP_TRY(hipEventElapsedTime(&t, c->events[2 * p], c->events[2 * p + 1]));
		ms += t;
	}
	stats->kernel_ms = ms;
	ptx_kernel_timing& tm = c->timing;
	tm.pipeline = wavefront ? 1u : 0u;
	tm.pool_pairs = wavefront ? plan.W.pool_cap : 0;
	tm.workspace_bytes = wavefront ? wf_workspace_bytes(c) : c->queues.cap + c->spill.cap;
	if (!wavefront) { tm.fused_ms = ms; tm.fused_launches = n_pass; }
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
	                                           "list_append", "shade_hit", "vertex_miss", "vertex_back_face", "vertex_last", "vertex_full"};
	for (int k = 0; k < kProfRegions; k++)
		fprintf(stderr, "PROF %-16s trips %12llu lanes %14llu  util %.3f  trips/64rays %.3f\n", names[k], prof[2 * k], prof[2 * k + 1],
		        prof[2 * k] ? (double)prof[2 * k + 1] / (64.0 * prof[2 * k]) : 0.0, (double)prof[2 * k] / ((double)rays / 64.0));
#endif
	return PTX_OK;
}

// what every render entry point refuses in a cfg, decided before any device work; -> the rectangle
int render_rect(const ptx_render_cfg* cfg, uint32_t& x0, uint32_t& y0, uint32_t& w, uint32_t& h) {
	if (!cfg->W || !cfg->H) return set_err(PTX_ERR_INVALID, "ptx_render: W and H must be > 0");   // bounces = 0 is legal: a black frame (renderer.cpp:438-439)
	x0 = cfg->x0; y0 = cfg->y0; w = cfg->w; h = cfg->h;
	if (w == 0 && h == 0) { x0 = 0; y0 = 0; w = cfg->W; h = cfg->H; }
	if (!w || !h || (uint64_t)x0 + w > cfg->W || (uint64_t)y0 + h > cfg->H) return set_err(PTX_ERR_INVALID, "ptx_render: tile outside the image");
	if (cfg->bounces > 0xFFFFu) return set_err(PTX_ERR_INVALID, "ptx_render: bounces > 65535");
	if (cfg->integrator > PTX_INTEGRATOR_WORKER) return set_err(PTX_ERR_INVALID, "ptx_render: unknown integrator");
	if (cfg->shard_count > 1 && cfg->shard_index >= cfg->shard_count) return set_err(PTX_ERR_INVALID, "ptx_render: shard_index >= shard_count");
	if ((uint64_t)w * h > 0x7FFFFFFFull) return set_err(PTX_ERR_INVALID, "ptx_render: tile too large");
	return PTX_OK;
}

// An explicit device list of tile-local pixel indices for a pass to render in place of pixel_list()'s (ptx_render_adaptive's active list)
struct PixelSubset {
	const uint32_t* d_pixels;
	uint32_t n_pixels;
};

// The caller holds the context's mutex and has set its device.
int render_frame_locked(ptx_scene* sc, const ptx_render_cfg* cfg, float* accum, uint8_t* claimed, ptx_render_stats* stats, const PixelSubset* subset) {
	uint32_t x0, y0, w, h;
	if (const int rc = render_rect(cfg, x0, y0, w, h); rc != PTX_OK) return rc;
	ptx_ctx* c = sc->ctx;
	const uint64_t rect_pixels = (uint64_t)w * h;
	if (stats) *stats = ptx_render_stats{};
	if (cfg->spp == 0) return PTX_OK;
	uint64_t n_pixels = 0;
	const uint32_t* d_pixels = nullptr;
	if (subset) {
		n_pixels = subset->n_pixels;
		d_pixels = subset->d_pixels;
	} else if (const int rc = pixel_list(c, sc, cfg, x0, y0, w, h, n_pixels, d_pixels); rc != PTX_OK) return rc;
	if (n_pixels == 0) return PTX_OK;   // no tile of this shard meets the rectangle
	const uint32_t pass_spp = pass_size(cfg, n_pixels);
	if (pass_spp == 0) return set_err(PTX_ERR_INVALID, "ptx_render: tile too large for one pass");

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
	float4* d_accum = (float4*)accum;
	if (!dev_accum) {
		HIP_TRY(c->stage_a.ensure(rect_pixels * sizeof(float4)));
		d_accum = (float4*)c->stage_a.p;
		HIP_TRY(hipMemcpyAsync(d_accum, accum, rect_pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
	}
	uint8_t* d_claimed = claimed;
	if (claimed && !dev_accum) {
		HIP_TRY(c->stage_b.ensure(rect_pixels));
		d_claimed = (uint8_t*)c->stage_b.p;
		HIP_TRY(hipMemcpyAsync(d_claimed, claimed, rect_pixels, hipMemcpyHostToDevice, c->stream));
	}

	const uint32_t n_pass = (cfg->spp + pass_spp - 1) / pass_spp;
	if (stats)
		while (c->events.size() < 2 * (size_t)n_pass) {
			hipEvent_t ev;
			HIP_TRY(hipEventCreate(&ev));
			c->events.push_back(ev);
		}
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
		RenderParams P{};
		P.W = cfg->W; P.H = cfg->H; P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
		P.n_pixels = (uint32_t)n_pixels;
		P.sample0 = cfg->sample0 + p * pass_spp;
		P.pass_spp = std::min(pass_spp, cfg->spp - p * pass_spp);
		P.bounces = cfg->bounces;
		P.transparent = claimed ? 1u : 0u;
		P.n_paths = (uint64_t)P.pass_spp * n_pixels;
		P.seed_lo = cfg->seed_lo; P.seed_hi = cfg->seed_hi;
		memcpy(P.env, cfg->env, sizeof P.env);
		P.integrator = cfg->integrator;
		P.pixels = d_pixels;
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
		if (claimed) HIP_TRY(launch_resolve_claim(B.sample_rad, d_accum, d_claimed, d_pixels, P.n_pixels, P.pass_spp, P.sample0, c->stream));
		else HIP_TRY(launch_resolve(B.sample_rad, d_accum, d_pixels, P.n_pixels, P.pass_spp, c->stream));
	}
	if (!dev_accum) HIP_TRY(hipMemcpyAsync(accum, d_accum, rect_pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
	if (claimed && !dev_accum) HIP_TRY(hipMemcpyAsync(claimed, d_claimed, rect_pixels, hipMemcpyDeviceToHost, c->stream));
	if (stats || !dev_accum) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) return render_stats(c, (uint64_t)cfg->spp * n_pixels, n_pass, wavefront, plan, clk, wf_rays, stats);
	return PTX_OK;
}

// ptx_render (claimed == nullptr: `accum` receives sums) and ptx_render_transparent (`accum` and `claimed` are the reference's per-pixel
// blend state, advanced through the samples in order) — the same passes, a different resolve kernel behind each
int render_frame(ptx_scene* sc, const ptx_render_cfg* cfg, float* accum, uint8_t* claimed, ptx_render_stats* stats) {
	uint32_t x0, y0, w, h;
	if (const int rc = render_rect(cfg, x0, y0, w, h); rc != PTX_OK) return rc;
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	return render_frame_locked(sc, cfg, accum, claimed, stats, nullptr);
}

}  // namespace

int ptx_render(ptx_scene* sc, const ptx_render_cfg* cfg, float* accum, ptx_render_stats* stats) {
	if (!sc || !cfg || !accum) return set_err(PTX_ERR_INVALID, "ptx_render: NULL argument");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render: scene was created without a GPU context (no CPU path exists)");
	return render_frame(sc, cfg, accum, nullptr, stats);
}

int ptx_render_transparent(ptx_scene* sc, const ptx_render_cfg* cfg, float* pixel_rgba, uint8_t* claimed, ptx_render_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !pixel_rgba || !claimed) return set_err(PTX_ERR_INVALID, "ptx_render_transparent: NULL argument");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_transparent: PTX_INTEGRATOR_WORKER has no transparent-background mode here (the worker takes the alpha of the "
		                                    "path's last vertex and jitters sample 0 in this mode, and nothing pins that); use PTX_INTEGRATOR_LIB");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_transparent: scene was created without a GPU context (no CPU path exists)");
	if (is_device_ptr(pixel_rgba) != is_device_ptr(claimed)) return set_err(PTX_ERR_INVALID, "ptx_render_transparent: pixel_rgba and claimed must both be device or both be host memory");
	return render_frame(sc, cfg, pixel_rgba, claimed, stats);
}

namespace {

// Closest hits of the A.n rays of `A` (device memory) on the scene's own route — the routing body of ptx_intersect_batch, shared with
// ptx_render_aov: the queue-based pipeline in slices with its overflow / retry handling, or the fused kernel's traversal. The caller holds
// the context's mutex and has set the device.
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
		HIP_TRY(launch_intersect(sc->dev, A, sc->mode, sc->lds_bytes, grid, c->stream));
	}
	return PTX_OK;
}

}  // namespace

int ptx_intersect_batch(ptx_scene* sc, const ptx_rays* r, size_t n, const ptx_hits* hh) {
	if (!sc || !r || !hh) return set_err(PTX_ERR_INVALID, "ptx_intersect_batch: NULL argument");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_intersect_batch: scene was created without a GPU context (no CPU path exists)");
	if (n == 0) return PTX_OK;
	if (!r->ox || !r->oy || !r->oz || !r->dx || !r->dy || !r->dz || !hh->distance || !hh->surface || !hh->triangle || !hh->b0 || !hh->b1 || !hh->b2)
		return set_err(PTX_ERR_INVALID, "ptx_intersect_batch: required array is NULL");
	auto group_ok = [](const void* a, const void* b, const void* c) { return (!a && !b && !c) || (a && b && c); };
	if (!group_ok(hh->px, hh->py, hh->pz) || !group_ok(hh->nx, hh->ny, hh->nz) || ((hh->u != nullptr) != (hh->v != nullptr)))
		return set_err(PTX_ERR_INVALID, "ptx_intersect_batch: optional outputs must be given as whole groups");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	const bool dev = is_device_ptr(r->ox);
	IntersectArgs A{};
	A.n = n;
	const int n_out = 6 + (hh->px ? 3 : 0) + (hh->nx ? 3 : 0) + (hh->u ? 2 : 0);
	if (dev) {
		A.ox = r->ox; A.oy = r->oy; A.oz = r->oz; A.dx = r->dx; A.dy = r->dy; A.dz = r->dz;
		A.distance = hh->distance; A.surface = hh->surface; A.triangle = hh->triangle;
		A.b0 = hh->b0; A.b1 = hh->b1; A.b2 = hh->b2;
		A.px = hh->px; A.py = hh->py; A.pz = hh->pz; A.nx = hh->nx; A.ny = hh->ny; A.nz = hh->nz; A.u = hh->u; A.v = hh->v;
	} else {
		HIP_TRY(c->stage_a.ensure(6 * n * 4));
		HIP_TRY(c->stage_b.ensure((size_t)n_out * n * 4));
		float* in = (float*)c->stage_a.p;
		const float* src[6] = {r->ox, r->oy, r->oz, r->dx, r->dy, r->dz};
		for (int k = 0; k < 6; k++) HIP_TRY(hipMemcpyAsync(in + k * n, src[k], n * 4, hipMemcpyHostToDevice, c->stream));
		A.ox = in; A.oy = in + n; A.oz = in + 2 * n; A.dx = in + 3 * n; A.dy = in + 4 * n; A.dz = in + 5 * n;
		float* o = (float*)c->stage_b.p;
		A.distance = o; A.surface = (int32_t*)(o + n); A.triangle = (int32_t*)(o + 2 * n);
		A.b0 = o + 3 * n; A.b1 = o + 4 * n; A.b2 = o + 5 * n;
		size_t k = 6;
		if (hh->px) { A.px = o + k * n; A.py = o + (k + 1) * n; A.pz = o + (k + 2) * n; k += 3; }
		if (hh->nx) { A.nx = o + k * n; A.ny = o + (k + 1) * n; A.nz = o + (k + 2) * n; k += 3; }
		if (hh->u) { A.u = o + k * n; A.v = o + (k + 1) * n; }
	}
	if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
	if (!dev) {
		void* dst[14] = {hh->distance, hh->surface, hh->triangle, hh->b0, hh->b1, hh->b2, hh->px, hh->py, hh->pz, hh->nx, hh->ny, hh->nz, hh->u, hh->v};
		const void* srcs[14] = {A.distance, A.surface, A.triangle, A.b0, A.b1, A.b2, A.px, A.py, A.pz, A.nx, A.ny, A.nz, A.u, A.v};
		for (int k = 0; k < 14; k++)
			if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], srcs[k], n * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	return PTX_OK;
}

namespace {

// samples of every pixel per AOV pass. The workspace holds two ray streams, the hits and two records per sample (kAovSampleBytes), so the
// default bounds a pass by samples, not by the frame: 32 Mi (16 spp of a 1080p frame, 3.8 GB)
constexpr size_t kAovSampleBytes = (2 * 8 + 6 + 8) * 4;
uint32_t aov_pass_size(const ptx_render_cfg* cfg, uint64_t n_pixels) {
	uint32_t pass_spp = cfg->spp_per_pass ? cfg->spp_per_pass : (uint32_t)std::max<uint64_t>(1, (32ull << 20) / n_pixels);
	pass_spp = std::min(pass_spp, cfg->spp);
	while ((uint64_t)pass_spp * n_pixels > 0xFFFFFFFFull) pass_spp--;   // sample ids are 32-bit
	return pass_spp;
}

}  // namespace

int ptx_render_aov(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_aov_buffers* out, ptx_render_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !out) return set_err(PTX_ERR_INVALID, "ptx_render_aov: NULL argument");
	if (!out->albedo_cov && !out->normal_depth) return set_err(PTX_ERR_INVALID, "ptx_render_aov: both buffers are NULL (at least one must be given)");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_aov: PTX_INTEGRATOR_WORKER has no guide buffers here (the worker's opacity handling and its un-jittered "
		                                    "sample 0 are not pinned); use PTX_INTEGRATOR_LIB");
	if (cfg->integrator > PTX_INTEGRATOR_WORKER) return set_err(PTX_ERR_INVALID, "ptx_render_aov: unknown integrator");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_aov: scene was created without a GPU context (no CPU path exists)");
	if (!cfg->W || !cfg->H) return set_err(PTX_ERR_INVALID, "ptx_render_aov: W and H must be > 0");
	uint32_t x0 = cfg->x0, y0 = cfg->y0, w = cfg->w, h = cfg->h;
	if (w == 0 && h == 0) { x0 = 0; y0 = 0; w = cfg->W; h = cfg->H; }
	if (!w || !h || (uint64_t)x0 + w > cfg->W || (uint64_t)y0 + h > cfg->H) return set_err(PTX_ERR_INVALID, "ptx_render_aov: tile outside the image");
	if (cfg->shard_count > 1 && cfg->shard_index >= cfg->shard_count) return set_err(PTX_ERR_INVALID, "ptx_render_aov: shard_index >= shard_count");
	const uint64_t rect_pixels = (uint64_t)w * h;
	if (rect_pixels > 0x7FFFFFFFull) return set_err(PTX_ERR_INVALID, "ptx_render_aov: tile too large");
	const bool dev_out = is_device_ptr(out->albedo_cov ? out->albedo_cov : out->normal_depth);
	if (out->albedo_cov && out->normal_depth && is_device_ptr(out->normal_depth) != dev_out)
		return set_err(PTX_ERR_INVALID, "ptx_render_aov: albedo_cov and normal_depth must both be device or both be host memory");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_render_stats{};
	if (cfg->spp == 0) return PTX_OK;
	uint64_t n_pixels = 0;
	const uint32_t* d_pixels = nullptr;
	if (const int rc = pixel_list(c, sc, cfg, x0, y0, w, h, n_pixels, d_pixels); rc != PTX_OK) return rc;
	if (n_pixels == 0) return PTX_OK;   // no tile of this shard meets the rectangle
	const uint32_t pass_spp = aov_pass_size(cfg, n_pixels);
	if (pass_spp == 0) return set_err(PTX_ERR_INVALID, "ptx_render_aov: tile too large for one pass");

	// workspace of one pass of `cap` samples: [256 B: live counts][stream 0][stream 1][hits][records]
	const size_t cap = ((size_t)pass_spp * n_pixels + 3) & ~(size_t)3;   // array stride: keeps the float4 records 16-byte aligned
	HIP_TRY(c->aov.ensure(256 + cap * kAovSampleBytes));
	uint32_t* const live_count = (uint32_t*)c->aov.p;
	float* f = (float*)((char*)c->aov.p + 256);
	AovStream st[2];
	for (AovStream& s : st) {
		s.ox = f; s.oy = f + cap; s.oz = f + 2 * cap; s.dx = f + 3 * cap; s.dy = f + 4 * cap; s.dz = f + 5 * cap;
		s.id = (uint32_t*)(f + 6 * cap); s.pass = (uint32_t*)(f + 7 * cap);
		f += 8 * cap;
	}
	float* const hits = f;
	float4* const rec = (float4*)(f + 6 * cap);

	float4* d_albedo = (float4*)out->albedo_cov;
	float4* d_normal = (float4*)out->normal_depth;
	if (!dev_out) {
		if (out->albedo_cov) {
			HIP_TRY(c->stage_a.ensure(rect_pixels * sizeof(float4)));
			d_albedo = (float4*)c->stage_a.p;
			HIP_TRY(hipMemcpyAsync(d_albedo, out->albedo_cov, rect_pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
		}
		if (out->normal_depth) {
			HIP_TRY(c->stage_b.ensure(rect_pixels * sizeof(float4)));
			d_normal = (float4*)c->stage_b.p;
			HIP_TRY(hipMemcpyAsync(d_normal, out->normal_depth, rect_pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
		}
	}

	const uint32_t n_pass = (cfg->spp + pass_spp - 1) / pass_spp;
	if (stats)
		while (c->events.size() < 2 * (size_t)n_pass) {
			hipEvent_t ev;
			HIP_TRY(hipEventCreate(&ev));
			c->events.push_back(ev);
		}
	const bool follow = sc->dev.any_alpha != 0;   // some material can pass a sample through: the live count decides when a pass is over
	uint64_t rays = 0;
	for (uint32_t p = 0; p < n_pass; p++) {
		RenderParams P{};
		P.W = cfg->W; P.H = cfg->H; P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
		P.n_pixels = (uint32_t)n_pixels;
		P.sample0 = cfg->sample0 + p * pass_spp;
		P.pass_spp = std::min(pass_spp, cfg->spp - p * pass_spp);
		P.n_paths = (uint64_t)P.pass_spp * n_pixels;
		P.seed_lo = cfg->seed_lo; P.seed_hi = cfg->seed_hi;
		P.integrator = PTX_INTEGRATOR_LIB;
		P.pixels = d_pixels;
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		HIP_TRY(launch_aov_generate(sc->dev, P, st[0], (uint32_t)P.n_paths, c->stream));
		uint32_t live = (uint32_t)P.n_paths;
		for (uint32_t round = 0; live != 0; round++) {
			AovStream in = st[round & 1u];
			if (round == 0) { in.id = nullptr; in.pass = nullptr; }   // entry i is sample i
			IntersectArgs A{};
			A.n = live;
			A.ox = in.ox; A.oy = in.oy; A.oz = in.oz; A.dx = in.dx; A.dy = in.dy; A.dz = in.dz;
			A.distance = hits; A.surface = (int32_t*)(hits + cap); A.triangle = (int32_t*)(hits + 2 * cap);
			A.b0 = hits + 3 * cap; A.b1 = hits + 4 * cap; A.b2 = hits + 5 * cap;
			if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
			rays += live;
			const AovHits H{A.surface, A.triangle, A.b1, A.b2};
			uint32_t* const n_out = live_count + (round & 1u);
			if (follow) HIP_TRY(hipMemsetAsync(n_out, 0, 4, c->stream));
			HIP_TRY(launch_aov_shade(sc->dev, P, in, H, live, st[(round + 1u) & 1u], n_out, rec, cap, c->stream));
			if (!follow) break;
			HIP_TRY(hipMemcpyAsync(&live, n_out, 4, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
		}
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		HIP_TRY(launch_aov_resolve(rec, cap, d_albedo, d_normal, d_pixels, P.n_pixels, P.pass_spp, c->stream));
	}
	if (!dev_out) {
		if (out->albedo_cov) HIP_TRY(hipMemcpyAsync(out->albedo_cov, d_albedo, rect_pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
		if (out->normal_depth) HIP_TRY(hipMemcpyAsync(out->normal_depth, d_normal, rect_pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
	}
	if (stats || !dev_out) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) {
		stats->rays = rays;
		stats->samples = (uint64_t)cfg->spp * n_pixels;
		stats->passes = n_pass;
		for (uint32_t p = 0; p < n_pass; p++) {
			float t = 0;
			HIP_TRY(hipEventElapsedTime(&t, c->events[2 * p], c->events[2 * p + 1]));
			stats->kernel_ms += t;
		}
	}
	return PTX_OK;
}

namespace {

// words per sample of ptx_render_nee's workspace: two path streams (12 each), the hits (6), the radiance record (4), the shadow stream
// (2 x 6 rays + 2 x 6 hits) and the per-path shadow records (10)
constexpr size_t kNeeSampleWords = 2 * 12 + 6 + 4 + 2 * 6 + 2 * 6 + 10;
// samples of every pixel per pass: by default 16 Mi samples (8 spp of a 1080p frame, 4.6 GB); at most 2^30, so that the positions of
// a round's shadow rays (two per path at most) stay below 2^31
uint32_t nee_pass_size(const ptx_render_cfg* cfg, uint64_t n_pixels) {
	uint32_t pass_spp = cfg->spp_per_pass ? cfg->spp_per_pass : (uint32_t)std::max<uint64_t>(1, (16ull << 20) / n_pixels);
	pass_spp = std::min(pass_spp, cfg->spp);
	while ((uint64_t)pass_spp * n_pixels > 0x3FFFFFFFull) pass_spp--;
	return pass_spp;
}

}  // namespace

int ptx_render_nee(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_nee_cfg* ncfg, float* accum, ptx_nee_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !accum) return set_err(PTX_ERR_INVALID, "ptx_render_nee: NULL argument");
	const uint32_t flags = ncfg ? ncfg->flags : 0u;
	if (flags & ~(uint32_t)PTX_NEE_NO_LIGHT_SAMPLES) return set_err(PTX_ERR_INVALID, "ptx_render_nee: unknown flag");
	if (cfg->integrator == PTX_INTEGRATOR_WORKER)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_nee: PTX_INTEGRATOR_WORKER has no light sampling here (the estimator is defined on PTX_INTEGRATOR_LIB's vertex)");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_nee: scene was created without a GPU context (no CPU path exists)");
	uint32_t x0, y0, w, h;
	if (const int rc = render_rect(cfg, x0, y0, w, h); rc != PTX_OK) return rc;
	const uint64_t rect_pixels = (uint64_t)w * h;
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) { *stats = ptx_nee_stats{}; c->timing = ptx_kernel_timing{}; c->timing.pipeline = use_wavefront(sc) ? 1u : 0u; }
	const ptx_scene::LightList& ll = *build_lights(sc);
	const uint32_t n_lights = (uint32_t)ll.cdf.size();
	if (stats) { stats->n_lights = n_lights; stats->light_area = ll.area; }
	if (cfg->spp == 0) return PTX_OK;
	uint64_t n_pixels = 0;
	const uint32_t* d_pixels = nullptr;
	if (const int rc = pixel_list(c, sc, cfg, x0, y0, w, h, n_pixels, d_pixels); rc != PTX_OK) return rc;
	if (n_pixels == 0) return PTX_OK;   // no tile of this shard meets the rectangle
	const uint32_t pass_spp = nee_pass_size(cfg, n_pixels);
	if (pass_spp == 0) return set_err(PTX_ERR_INVALID, "ptx_render_nee: tile too large for one pass");

	NeeLights Lt{};
	if (n_lights && !(flags & PTX_NEE_NO_LIGHT_SAMPLES)) {
		if (!sc->lights.on_device) {
			HIP_TRY(sc->d_light_tris.ensure(ll.tris.size() * 4));
			HIP_TRY(sc->d_light_cdf.ensure(ll.cdf.size() * 4));
			HIP_TRY(sc->d_light_geom.ensure(ll.geom.size() * 4));
			HIP_TRY(sc->d_light_first.ensure(ll.surf_first.size() * 4));
			HIP_TRY(hipMemcpyAsync(sc->d_light_tris.p, ll.tris.data(), ll.tris.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipMemcpyAsync(sc->d_light_cdf.p, ll.cdf.data(), ll.cdf.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipMemcpyAsync(sc->d_light_geom.p, ll.geom.data(), ll.geom.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipMemcpyAsync(sc->d_light_first.p, ll.surf_first.data(), ll.surf_first.size() * 4, hipMemcpyHostToDevice, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			sc->lights.on_device = true;
		}
		Lt.tris = (const uint2*)sc->d_light_tris.p; Lt.cdf = (const float*)sc->d_light_cdf.p; Lt.geom = (const float4*)sc->d_light_geom.p;
		Lt.surf_first = (const int32_t*)sc->d_light_first.p; Lt.n = n_lights; Lt.area = ll.area;
	}

	// workspace of one pass of `cap` samples: [256 B: counters][radiance records][stream 0][stream 1][hits][shadow rays][shadow hits][shadow records]
	const size_t cap = ((size_t)pass_spp * n_pixels + 3) & ~(size_t)3;   // array stride: keeps every array 16-byte aligned
	HIP_TRY(c->aov.ensure(256 + cap * kNeeSampleWords * 4));
	uint32_t* const cnt = (uint32_t*)c->aov.p;
	float* f = (float*)((char*)c->aov.p + 256);
	float4* const Lrec = (float4*)f;
	f += 4 * cap;
	NeeStream st[2];
	for (NeeStream& s : st) {
		s.ox = f; s.oy = f + cap; s.oz = f + 2 * cap; s.dx = f + 3 * cap; s.dy = f + 4 * cap; s.dz = f + 5 * cap;
		s.tx = f + 6 * cap; s.ty = f + 7 * cap; s.tz = f + 8 * cap; s.pp = f + 9 * cap;
		s.id = (uint32_t*)(f + 10 * cap); s.dp = (uint32_t*)(f + 11 * cap);
		f += 12 * cap;
	}
	float* const hits = f;
	f += 6 * cap;
	NeeShadow W{};
	W.ox = f; W.oy = f + 2 * cap; W.oz = f + 4 * cap; W.dx = f + 6 * cap; W.dy = f + 8 * cap; W.dz = f + 10 * cap;
	f += 12 * cap;
	float* const shits = f;
	f += 12 * cap;
	W.sx = f; W.sy = f + cap; W.sz = f + 2 * cap; W.lx = f + 3 * cap; W.ly = f + 4 * cap; W.lz = f + 5 * cap;
	W.sun_pos = (uint32_t*)(f + 6 * cap); W.light_pos = (uint32_t*)(f + 7 * cap); W.exp_surf = (uint32_t*)(f + 8 * cap); W.exp_tri = (uint32_t*)(f + 9 * cap);

	const bool dev_accum = is_device_ptr(accum);
	float4* d_accum = (float4*)accum;
	if (!dev_accum) {
		HIP_TRY(c->stage_a.ensure(rect_pixels * sizeof(float4)));
		d_accum = (float4*)c->stage_a.p;
		HIP_TRY(hipMemcpyAsync(d_accum, accum, rect_pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
	}
	const uint32_t n_pass = (cfg->spp + pass_spp - 1) / pass_spp;
	if (stats)
		while (c->events.size() < 2 * (size_t)n_pass) {
			hipEvent_t ev;
			HIP_TRY(hipEventCreate(&ev));
			c->events.push_back(ev);
		}
	HIP_TRY(hipMemsetAsync(cnt, 0, 256, c->stream));
	// a lit shadow catcher's pass-through ray is appended by the settle kernel: only then is the live count read a second time in a round
	const bool catchers = sc->dev.any_alpha != 0 && sc->dev.sun.present != 0;
	uint64_t rays = 0;
	for (uint32_t p = 0; p < n_pass; p++) {
		RenderParams P{};
		P.W = cfg->W; P.H = cfg->H; P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
		P.n_pixels = (uint32_t)n_pixels;
		P.sample0 = cfg->sample0 + p * pass_spp;
		P.pass_spp = std::min(pass_spp, cfg->spp - p * pass_spp);
		P.bounces = cfg->bounces;
		P.n_paths = (uint64_t)P.pass_spp * n_pixels;
		P.seed_lo = cfg->seed_lo; P.seed_hi = cfg->seed_hi;
		memcpy(P.env, cfg->env, sizeof P.env);
		P.integrator = PTX_INTEGRATOR_LIB;
		P.pixels = d_pixels;
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p], c->stream));
		HIP_TRY(launch_nee_generate(sc->dev, P, st[0], Lrec, (uint32_t)P.n_paths, c->stream));
		uint32_t live = P.bounces > 0 ? (uint32_t)P.n_paths : 0u;
		for (uint32_t round = 0; live != 0; round++) {
			const NeeStream& in = st[round & 1u];
			const NeeStream& out = st[(round + 1u) & 1u];
			IntersectArgs A{};
			A.n = live;
			A.ox = in.ox; A.oy = in.oy; A.oz = in.oz; A.dx = in.dx; A.dy = in.dy; A.dz = in.dz;
			A.distance = hits; A.surface = (int32_t*)(hits + cap); A.triangle = (int32_t*)(hits + 2 * cap);
			A.b0 = hits + 3 * cap; A.b1 = hits + 4 * cap; A.b2 = hits + 5 * cap;
			if (const int rc = intersect_device(c, sc, A); rc != PTX_OK) return rc;
			rays += live;
			const NeeHits H{A.distance, A.surface, A.triangle, A.b1, A.b2};
			HIP_TRY(hipMemsetAsync(cnt, 0, 8, c->stream));
			HIP_TRY(launch_nee_shade(sc->dev, P, Lt, in, H, live, out, W, cnt, Lrec, c->stream));
			uint32_t got[2] = {0, 0};   // continuations, shadow rays
			HIP_TRY(hipMemcpyAsync(got, cnt, 8, hipMemcpyDeviceToHost, c->stream));
			HIP_TRY(hipStreamSynchronize(c->stream));
			if (got[0] > live || got[1] > 2ull * live) return set_err(PTX_ERR_HIP, "ptx_render_nee: a round appended more entries than its paths allow");
			if (got[1]) {
				IntersectArgs B{};
				B.n = got[1];
				B.ox = W.ox; B.oy = W.oy; B.oz = W.oz; B.dx = W.dx; B.dy = W.dy; B.dz = W.dz;
				B.distance = shits; B.surface = (int32_t*)(shits + 2 * cap); B.triangle = (int32_t*)(shits + 4 * cap);
				B.b0 = shits + 6 * cap; B.b1 = shits + 8 * cap; B.b2 = shits + 10 * cap;
				if (const int rc = intersect_device(c, sc, B); rc != PTX_OK) return rc;
				rays += got[1];
				const NeeHits SH{B.distance, B.surface, B.triangle, B.b1, B.b2};
				HIP_TRY(launch_nee_settle(in, live, W, SH, out, cnt, Lrec, c->stream));
				if (catchers) {
					HIP_TRY(hipMemcpyAsync(got, cnt, 4, hipMemcpyDeviceToHost, c->stream));
					HIP_TRY(hipStreamSynchronize(c->stream));
					if (got[0] > live) return set_err(PTX_ERR_HIP, "ptx_render_nee: a round appended more entries than its paths allow");
				}
			}
			live = got[0];
		}
		if (stats) HIP_TRY(hipEventRecord(c->events[2 * p + 1], c->stream));
		HIP_TRY(launch_resolve(Lrec, d_accum, d_pixels, P.n_pixels, P.pass_spp, c->stream));
	}
	if (!dev_accum) HIP_TRY(hipMemcpyAsync(accum, d_accum, rect_pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
	if (stats || !dev_accum) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) {
		unsigned long long ls[2] = {0, 0};
		HIP_TRY(hipMemcpy(ls, cnt + 2, 16, hipMemcpyDeviceToHost));
		stats->light_samples = ls[0]; stats->light_visible = ls[1];
		stats->render.rays = rays;
		stats->render.samples = (uint64_t)cfg->spp * n_pixels;
		stats->render.passes = n_pass;
		for (uint32_t p = 0; p < n_pass; p++) {
			float t = 0;
			HIP_TRY(hipEventElapsedTime(&t, c->events[2 * p], c->events[2 * p + 1]));
			stats->render.kernel_ms += t;
		}
	}
	return PTX_OK;
}

namespace {

// Which iterations (bit i = step 2^i) run the LDS-tiled a-trous kernel rather than the global gather: the faster of the two per step at
// 1920 x 1080 on the MI355X (profiles/EXPERIMENTS.md). PTX_DENOISE_TILED=<mask>: measurement switch. Both forms give the same bits.
constexpr uint32_t kDenoiseTiledSteps = 0x00;
uint32_t denoise_tiled_steps() {
	const char* e = getenv("PTX_DENOISE_TILED");
	return e && *e ? (uint32_t)strtoul(e, nullptr, 0) : kDenoiseTiledSteps;
}

}  // namespace

int ptx_denoise(ptx_ctx* c, const ptx_denoise_cfg* cfg, const float* accum_a, const float* accum_b, const ptx_aov_buffers* guides, float* out_rgba, ptx_denoise_stats* stats) {
	// every refusal below is decided before any device work
	if (!c || !cfg || !accum_a || !accum_b || !guides || !out_rgba) return set_err(PTX_ERR_INVALID, "ptx_denoise: NULL argument");
	if (!guides->albedo_cov || !guides->normal_depth) return set_err(PTX_ERR_INVALID, "ptx_denoise: both guide buffers are required");
	if (!cfg->W || !cfg->H || cfg->W > 16384 || cfg->H > 16384) return set_err(PTX_ERR_INVALID, "ptx_denoise: W and H must be in 1 .. 16384");
	if (!cfg->spp_a || !cfg->spp_b) return set_err(PTX_ERR_INVALID, "ptx_denoise: spp_a and spp_b must be > 0 (the noise estimate needs two half-frames)");
	if (cfg->iterations > 8) return set_err(PTX_ERR_INVALID, "ptx_denoise: at most 8 iterations");
	if (!(cfg->sigma_l >= 0.0f) || !(cfg->sigma_n >= 0.0f) || !(cfg->sigma_z >= 0.0f)) return set_err(PTX_ERR_INVALID, "ptx_denoise: a sigma is negative or NaN");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev || is_device_ptr(guides->albedo_cov) != dev || is_device_ptr(guides->normal_depth) != dev || is_device_ptr(out_rgba) != dev)
		return set_err(PTX_ERR_INVALID, "ptx_denoise: the five buffers must all be device or all be host memory");
	const uint32_t W = cfg->W, H = cfg->H, iterations = cfg->iterations ? cfg->iterations : 5u;
	const float sigma_l = cfg->sigma_l != 0.0f ? cfg->sigma_l : 4.0f, sigma_n = cfg->sigma_n != 0.0f ? cfg->sigma_n : 0.5f, sigma_z = cfg->sigma_z != 0.0f ? cfg->sigma_z : 0.1f;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_denoise_stats{};

	// workspace: [state 0][state 1][guide][remod], then the staging of the four host inputs; the staged output takes accum_a's place
	const size_t n = (size_t)W * H, bytes = n * sizeof(float4);
	const size_t ws_bytes = bytes * (dev ? 4 : 8);
	HIP_TRY(c->denoise.ensure(ws_bytes));
	float4* const ws = (float4*)c->denoise.p;
	float4 *const state[2] = {ws, ws + n}, *const guide = ws + 2 * n, *const remod = ws + 3 * n;
	const float4 *d_a = (const float4*)accum_a, *d_b = (const float4*)accum_b, *d_alb = (const float4*)guides->albedo_cov, *d_nd = (const float4*)guides->normal_depth;
	float4* d_out = (float4*)out_rgba;
	if (!dev) {
		const void* src[4] = {accum_a, accum_b, guides->albedo_cov, guides->normal_depth};
		for (int k = 0; k < 4; k++) HIP_TRY(hipMemcpyAsync(ws + (4 + k) * n, src[k], bytes, hipMemcpyHostToDevice, c->stream));
		d_a = ws + 4 * n; d_b = ws + 5 * n; d_alb = ws + 6 * n; d_nd = ws + 7 * n;
		d_out = ws + 4 * n;   // prepare has consumed the inputs before the last iteration writes
	}
	if (stats)
		while (c->events.size() < 2) {
			hipEvent_t ev;
			HIP_TRY(hipEventCreate(&ev));
			c->events.push_back(ev);
		}
	const uint32_t tiled = denoise_tiled_steps();
	if (stats) HIP_TRY(hipEventRecord(c->events[0], c->stream));
	HIP_TRY(launch_denoise_prepare(d_a, d_b, d_alb, d_nd, cfg->spp_a, cfg->spp_b, n, state[0], guide, remod, c->stream));
	HIP_TRY(launch_denoise_prefilter(state[0], guide, W, H, sigma_n, sigma_z, state[1], c->stream));
	for (uint32_t i = 0; i < iterations; i++) {
		const bool last = i + 1 == iterations;
		const float4* in = state[(i + 1) & 1u];
		HIP_TRY(launch_denoise_atrous(in, guide, remod, W, H, 1u << i, sigma_l, sigma_n, sigma_z, last, (tiled >> i) & 1u, last ? d_out : state[i & 1u], c->stream));
	}
	if (stats) HIP_TRY(hipEventRecord(c->events[1], c->stream));
	if (!dev) HIP_TRY(hipMemcpyAsync(out_rgba, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
	if (stats || !dev) HIP_TRY(hipStreamSynchronize(c->stream));
	if (stats) {
		float t = 0;
		HIP_TRY(hipEventElapsedTime(&t, c->events[0], c->events[1]));
		stats->kernel_ms = t;
		stats->iterations = iterations;
		stats->workspace_bytes = ws_bytes;
	}
	return PTX_OK;
}

namespace {

// One decision on device buffers (adaptive.hip), its count read back: the stream is synchronised. The caller holds the context's mutex.
// select_ms: nullptr, or where the HIP-event time of the decision kernels is added.
int adaptive_decide_locked(ptx_ctx* c, uint32_t w, uint32_t h, const float4* d_a, const float4* d_b, float threshold, uint8_t* d_done, uint32_t* d_pixels, uint32_t& n_active,
                           double* select_ms) {
	const size_t n = (size_t)w * h, tiles = (size_t)((w + kAdTile - 1) / kAdTile) * ((h + kAdTile - 1) / kAdTile), blocks = tiles * kAdBlocksPerTile;
	const size_t o_mask = pad16(n), o_boff = o_mask + blocks * 8, o_tcnt = o_boff + blocks * 4, o_toff = o_tcnt + pad16(tiles * 4), o_cnt = o_toff + pad16(tiles * 4);
	HIP_TRY(c->adaptive.ensure(o_cnt + 16));
	char* const ws = (char*)c->adaptive.p;
	const AdaptiveBuffers B{(uint8_t*)ws, (unsigned long long*)(ws + o_mask), (uint32_t*)(ws + o_boff), (uint32_t*)(ws + o_tcnt), (uint32_t*)(ws + o_toff), (uint32_t*)(ws + o_cnt)};
	if (select_ms)
		for (hipEvent_t& ev : c->adaptive_ev)
			if (!ev) HIP_TRY(hipEventCreate(&ev));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[0], c->stream));
	HIP_TRY(launch_adaptive_select(d_a, d_b, w, h, threshold, B, d_done, d_pixels, c->stream));
	if (select_ms) HIP_TRY(hipEventRecord(c->adaptive_ev[1], c->stream));
	HIP_TRY(hipMemcpyAsync(&n_active, B.n_active, 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (select_ms) {
		float t = 0;
		HIP_TRY(hipEventElapsedTime(&t, c->adaptive_ev[0], c->adaptive_ev[1]));
		*select_ms += t;
	}
	return PTX_OK;
}

}  // namespace

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
	const float4 *d_a = (const float4*)accum_a, *d_b = (const float4*)accum_b;
	uint8_t* d_done = done;
	uint32_t* d_pixels = pixels;
	if (!dev) {
		HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
		HIP_TRY(c->adaptive_state.ensure(n * 4 + pad16(n)));
		d_a = (const float4*)c->adaptive_stage.p; d_b = d_a + n;
		if (pixels) d_pixels = (uint32_t*)c->adaptive_state.p;
		d_done = (uint8_t*)c->adaptive_state.p + n * 4;
		HIP_TRY(hipMemcpyAsync((void*)d_a, accum_a, bytes, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync((void*)d_b, accum_b, bytes, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_done, done, n, hipMemcpyHostToDevice, c->stream));
	}
	uint32_t count = 0;
	if (const int rc = adaptive_decide_locked(c, w, h, d_a, d_b, threshold, d_done, d_pixels, count, nullptr); rc != PTX_OK) return rc;
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(done, d_done, n, hipMemcpyDeviceToHost, c->stream));
		if (pixels && count) HIP_TRY(hipMemcpyAsync(pixels, d_pixels, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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
	const float4 *d_a = (const float4*)accum_a, *d_b = (const float4*)accum_b;
	float4* d_out = (float4*)out_rgba;
	if (!dev) {
		HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
		float4* const st = (float4*)c->adaptive_stage.p;
		HIP_TRY(hipMemcpyAsync(st, accum_a, bytes, hipMemcpyHostToDevice, c->stream));
		if (accum_b) HIP_TRY(hipMemcpyAsync(st + n_pixels, accum_b, bytes, hipMemcpyHostToDevice, c->stream));
		d_a = st; d_b = accum_b ? st + n_pixels : nullptr; d_out = st;
	}
	HIP_TRY(launch_accum_mean(d_a, d_b, n_pixels, d_out, c->stream));
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(out_rgba, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	return PTX_OK;
}

int ptx_render_adaptive(ptx_scene* sc, const ptx_render_cfg* cfg, const ptx_adaptive_cfg* acfg, float* accum_a, float* accum_b, ptx_adaptive_stats* stats) {
	// every refusal below is decided before any device work
	if (!sc || !cfg || !acfg || !accum_a || !accum_b) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: NULL argument");
	if (acfg->min_spp < 2 || (acfg->min_spp & 1u)) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: min_spp must be even and >= 2 (each round is split into two halves)");
	if (acfg->step_spp & 1u) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: step_spp must be even (0 = min_spp)");
	if ((cfg->spp & 1u) || cfg->spp < acfg->min_spp) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: spp (the cap) must be even and >= min_spp");
	const uint32_t step = acfg->step_spp ? acfg->step_spp : acfg->min_spp;
	if ((uint64_t)1 + ((uint64_t)(cfg->spp - acfg->min_spp) + step - 1) / step > 4096) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: more than 4096 rounds");
	if (!(acfg->threshold >= 0.0f)) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: threshold is negative or NaN");
	if ((uint64_t)cfg->sample0 + cfg->spp > 0xFFFFFFFFull) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: sample0 + spp overflows");
	uint32_t x0, y0, w, h;
	if (const int rc = render_rect(cfg, x0, y0, w, h); rc != PTX_OK) return rc;
	if (w > kAdMaxSide || h > kAdMaxSide) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: the rectangle's sides must be at most 16384");
	if (cfg->shard_count > 1)
		return set_err(PTX_ERR_UNSUPPORTED, "ptx_render_adaptive: shard_count > 1 is not supported (the 3 x 3 block of the decision would need other shards' pixels); "
		                                    "split a frame over GPUs by rectangles instead");
	if (!sc->ctx) return set_err(PTX_ERR_NO_DEVICE, "ptx_render_adaptive: scene was created without a GPU context (no CPU path exists)");
	const bool dev = is_device_ptr(accum_a);
	if (is_device_ptr(accum_b) != dev) return set_err(PTX_ERR_INVALID, "ptx_render_adaptive: accum_a and accum_b must both be device or both be host memory");
	ptx_ctx* c = sc->ctx;
	std::lock_guard<std::mutex> lk(c->mu);
	HIP_TRY(hipSetDevice(c->device));
	if (stats) *stats = ptx_adaptive_stats{};

	const size_t n = (size_t)w * h, bytes = n * sizeof(float4);
	float4 *d_a = (float4*)accum_a, *d_b = (float4*)accum_b;
	if (!dev) {   // staged once for the whole call
		HIP_TRY(c->adaptive_stage.ensure(2 * bytes));
		d_a = (float4*)c->adaptive_stage.p; d_b = d_a + n;
		HIP_TRY(hipMemcpyAsync(d_a, accum_a, bytes, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(d_b, accum_b, bytes, hipMemcpyHostToDevice, c->stream));
	}
	HIP_TRY(c->adaptive_state.ensure(n * 4 + pad16(n)));
	uint32_t* const d_list = (uint32_t*)c->adaptive_state.p;
	uint8_t* const d_done = (uint8_t*)c->adaptive_state.p + n * 4;
	HIP_TRY(hipMemsetAsync(d_done, 0, n, c->stream));

	ptx_render_cfg half = *cfg;
	half.x0 = x0; half.y0 = y0; half.w = w; half.h = h;
	PixelSubset active{d_list, 0};
	uint32_t given = 0, rounds = 0, n_active = 0;
	double select_ms = 0;
	while (given < cfg->spp) {
		const uint32_t k = rounds == 0 ? acfg->min_spp : std::min(step, cfg->spp - given);
		float4* const target[2] = {d_a, d_b};
		for (uint32_t part = 0; part < 2; part++) {   // the first half of the round's samples into A, the second into B
			half.sample0 = cfg->sample0 + given + part * (k / 2);
			half.spp = k / 2;
			ptx_render_stats st{};
			if (const int rc = render_frame_locked(sc, &half, (float*)target[part], nullptr, stats ? &st : nullptr, rounds == 0 ? nullptr : &active); rc != PTX_OK) return rc;
			if (stats) {
				stats->render.rays += st.rays; stats->render.samples += st.samples; stats->render.passes += st.passes; stats->render.kernel_ms += st.kernel_ms;
			}
		}
		given += k;
		rounds++;
		if (const int rc = adaptive_decide_locked(c, w, h, d_a, d_b, acfg->threshold, d_done, d_list, n_active, stats ? &select_ms : nullptr); rc != PTX_OK) return rc;
		active.n_pixels = n_active;
		if (n_active == 0) break;
	}
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(accum_a, d_a, bytes, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipMemcpyAsync(accum_b, d_b, bytes, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	if (stats) {
		stats->rounds = rounds;
		stats->active_last = n_active;
		stats->select_ms = select_ms;
	}
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
	const float* d_in = in;
	float* d_out = out;
	if (!dev) {
		HIP_TRY(c->stage_a.ensure(n * 14 * 4));
		HIP_TRY(c->stage_b.ensure(n * 15 * 4));
		HIP_TRY(hipMemcpyAsync(c->stage_a.p, in, n * 14 * 4, hipMemcpyHostToDevice, c->stream));
		d_in = (const float*)c->stage_a.p;
		d_out = (float*)c->stage_b.p;
	}
	HIP_TRY(launch_pbr_eval(d_in, d_out, n, c->stream));
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(out, d_out, n * 15 * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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
	const float* d_in = ndc_ratio;
	float* d_out = rays;
	if (!dev) {
		HIP_TRY(c->stage_a.ensure(n * 3 * 4));
		HIP_TRY(c->stage_b.ensure(n * 6 * 4));
		HIP_TRY(hipMemcpyAsync(c->stage_a.p, ndc_ratio, n * 3 * 4, hipMemcpyHostToDevice, c->stream));
		d_in = (const float*)c->stage_a.p;
		d_out = (float*)c->stage_b.p;
	}
	HIP_TRY(launch_camera_rays(sc->dev, d_in, d_out, n, c->stream));
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(rays, d_out, n * 6 * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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
	const int32_t* d_surf = surface;
	const float* d_uv = uv;
	float* d_out = out;
	if (!dev) {
		HIP_TRY(c->stage_a.ensure(n * 12));
		HIP_TRY(c->stage_b.ensure(n * 12 * 4));
		HIP_TRY(hipMemcpyAsync(c->stage_a.p, uv, n * 8, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync((char*)c->stage_a.p + n * 8, surface, n * 4, hipMemcpyHostToDevice, c->stream));
		d_uv = (const float*)c->stage_a.p;
		d_surf = (const int32_t*)((const char*)c->stage_a.p + n * 8);
		d_out = (float*)c->stage_b.p;
	}
	HIP_TRY(launch_material_eval(sc->dev, d_surf, d_uv, n, d_out, c->stream));
	if (!dev) {
		HIP_TRY(hipMemcpyAsync(out, d_out, n * 12 * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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
	const float4* d_in = (const float4*)accum;
	uchar4* d_out = (uchar4*)rgba8;
	if (!dev_in) {
		HIP_TRY(c->stage_a.ensure(n * 16));
		HIP_TRY(hipMemcpyAsync(c->stage_a.p, accum, n * 16, hipMemcpyHostToDevice, c->stream));
		d_in = (const float4*)c->stage_a.p;
	}
	if (!dev_out) {
		HIP_TRY(c->stage_b.ensure(n * 4));
		d_out = (uchar4*)c->stage_b.p;
	}
	if (!c->srgb_thr.p) {
		float thr[256];
		srgb_thresholds(thr);
		HIP_TRY(c->srgb_thr.ensure(sizeof thr));
		HIP_TRY(hipMemcpy(c->srgb_thr.p, thr, sizeof thr, hipMemcpyHostToDevice));
	}
	HIP_TRY(launch_tonemap(d_in, (uint32_t)n, (float)spp, (const float*)c->srgb_thr.p, d_out, c->stream));
	if (!dev_out) {
		HIP_TRY(hipMemcpyAsync(rgba8, d_out, n * 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
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

}  // extern "C"
