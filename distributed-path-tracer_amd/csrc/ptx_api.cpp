// C ABI of libptx_hip.so (declared in include/ptx.h). Host glue only: contexts, scene upload, pass scheduling, staging of host buffers.
// This file: contexts and scenes; api_render.cpp: the render entry points; api_batch.cpp: the batch calls; api_internal.hpp: what they share.
// All arithmetic of the hot path lives in kernels.hip; there is no CPU fallback — GPU entry points fail with PTX_ERR_NO_DEVICE when no HIP
// device exists.
#include <algorithm>
#include <cmath>
#include <deque>

#include "api_internal.hpp"

namespace {
thread_local std::string g_err;
}
int set_err(int code, const std::string& m) { g_err = m; return code; }

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

namespace {

constexpr size_t kLdsBudget = 160 * 1024;   // per-CU LDS on gfx950; one workgroup may take all of it
constexpr size_t kLeafOrderMaxBytes = (size_t)1 << 40;   // never reached: see decide_mode

// Residency plan -> kernel family. PTX_FORCE_GLOBAL / PTX_NO_HYBRID: measurement switches.
void decide_mode(ptx_scene* sc) {
	FlatScene& h = sc->host;
	// PTX_LDS_LEAF_ORDER=0/1: the resident copy all ref-indexed / leaf-ordered where it is cheap (the default); PTX_LDS_BUDGET: a smaller
	// budget for the residency plan, in bytes (measurement and tests; read once, here); PTX_KD_SHAPES=0/1: no shape bits in lds_root, so
	// that every walk is the general one / the shape bits of the leaf-ordered trees (the default)
	if (sc->lds_leaf_order < 0) {
		const char* e = getenv("PTX_LDS_LEAF_ORDER");
		sc->lds_leaf_order = (e && e[0] == '0') ? 0 : 1;
		const char* k = getenv("PTX_KD_SHAPES");
		sc->kd_shapes = (k && k[0] == '0') ? 0 : 1;
		sc->lds_budget = kLdsBudget;
		if (const char* b = getenv("PTX_LDS_BUDGET")) sc->lds_budget = std::min<size_t>(kLdsBudget, (size_t)strtoull(b, nullptr, 10));
	}
	plan_residency(h, sc->lds_budget, sc->lds_leaf_order != 0, sc->kd_shapes != 0);
	if (getenv("PTX_FORCE_GLOBAL") || h.n_resident == 0) sc->mode = MODE_GLOBAL;
	else if (h.n_resident == h.surfaces.size()) sc->mode = MODE_LDS;
	else sc->mode = getenv("PTX_NO_HYBRID") ? MODE_GLOBAL : MODE_HYBRID;
	if (sc->mode == MODE_GLOBAL) {
		for (auto& sr : h.surfaces) sr.lds_root = 0xFFFFFFFFu;
		for (auto& a : h.surf_aux) a.flags &= ~kAuxChainBit;   // a flag of resident trees only
	}
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
	HIP_TRY(up(sc->d_surf_aux, h.surf_aux.data(), h.surf_aux.size() * sizeof(UnitAux), h.surf_aux.size() * sizeof(UnitAux)));
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
	{   // the aperture table: always the full 33 corners, so that ptx_scene_set_camera never has to allocate
		const std::vector<float> lens = lens_table(h.camera);
		HIP_TRY(up(sc->d_lens, lens.data(), lens.size() * 4, (kLensMaxBlades + 1) * 8));
	}
	HIP_TRY(hipStreamSynchronize(c->stream));
	DevScene& d = sc->dev;
	d.models = (const ModelRec*)sc->d_models.p;
	d.surfaces = (const SurfaceRec*)sc->d_surfaces.p;
	d.surf_aux = (const UnitAux*)sc->d_surf_aux.p;
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
	d.lens = (const float2*)sc->d_lens.p;
	return PTX_OK;
}

void release_scene_buffers(ptx_scene* sc) {
	for (DevBuf* b : {&sc->d_models, &sc->d_surfaces, &sc->d_materials, &sc->d_nodes, &sc->d_refs, &sc->d_tris, &sc->d_shade, &sc->d_tex,
	                  &sc->d_texels, &sc->d_texels_f, &sc->d_lut, &sc->d_spaces, &sc->d_model_space, &sc->d_surf_aux, &sc->d_wf_order, &sc->d_res_nodes, &sc->d_res_refs, &sc->d_res_tris, &sc->d_hot,
	                  &sc->d_light_tris, &sc->d_light_cdf, &sc->d_light_geom, &sc->d_light_first, &sc->d_light_tree, &sc->d_light_path, &sc->d_env_row, &sc->d_env_cell, &sc->d_punctual, &sc->d_punctual_cdf, &sc->d_punctual_tree, &sc->d_lens, &sc->d_motion})
		b->release();
	sc->lights.on_device = false;
	sc->env_table.on_device = false;
	sc->punctual.on_device = false;
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

// The ray spaces and the motion table of the scene's motion state, in stream order into buffers the scene owns: what ptx_scene_set_motion
// and the calls that end a motion change on the device. No tree, no triangle, no shade record goes up.
int upload_motion(ptx_scene* sc) {
	ptx_ctx* c = sc->ctx;
	HIP_TRY(hipSetDevice(c->device));
	const FlatScene& h = sc->host;
	HIP_TRY(hipStreamSynchronize(c->stream));   // a buffer that grows is freed: nothing queued may still read it
	auto up = [&](DevBuf& b, const void* src, size_t bytes) -> hipError_t {
		hipError_t e = b.ensure(std::max<size_t>(bytes, 16));
		if (e != hipSuccess) return e;
		return bytes ? hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
	};
	HIP_TRY(up(sc->d_spaces, h.spaces.data(), h.spaces.size() * sizeof(SpaceRec)));
	HIP_TRY(up(sc->d_model_space, h.model_space.data(), h.model_space.size() * 4));
	sc->dev_motion = DevMotion{};
	std::vector<float> table;
	if (h.motion.set && h.motion.any_model()) {
		const size_t n = h.models.size();
		table.resize(25 * n);
		memcpy(table.data(), h.motion.begin_xform.data(), 48 * n);
		memcpy(table.data() + 12 * n, h.model_xform.data(), 48 * n);
		memcpy(table.data() + 24 * n, h.motion.moved.data(), 4 * n);
		HIP_TRY(up(sc->d_motion, table.data(), table.size() * 4));
		const float* base = (const float*)sc->d_motion.p;
		sc->dev_motion = DevMotion{base, base + 12 * n, (const uint32_t*)(base + 24 * n)};
	}
	HIP_TRY(hipStreamSynchronize(c->stream));   // `table` is a local
	sc->dev.spaces = (const SpaceRec*)sc->d_spaces.p;
	sc->dev.model_space = (const uint32_t*)sc->d_model_space.p;
	sc->dev.n_spaces = (uint32_t)h.spaces.size();
	return PTX_OK;
}

// Ends the scene's motion: the inspection arrays are empty again, the ray spaces are the static scene's, and the light list (which left
// out the moving models) is dropped. The caller holds the context's mutex on a scene with one. -> whether ray spaces changed.
bool drop_motion(ptx_scene* sc) {
	FlatScene& h = sc->host;
	if (!h.motion.set) return false;
	const bool had_models = h.motion.any_model();
	h.motion = FlatScene::Motion{};
	sc->dev_motion = DevMotion{};
	if (!had_models) return false;
	assign_ray_spaces(h);
	std::lock_guard<std::mutex> tl(sc->lights_mu);
	sc->lights = ptx_scene::LightList{};
	return true;
}

}  // namespace

int refuse_motion(const char* who) {
	return set_err(PTX_ERR_UNSUPPORTED, std::string(who) + ": the scene's motion is active (ptx_scene_set_motion) and this call knows no time per sample: it would render the "
	                                    "scene at u = 1 only. Render the blurred frame with ptx_render_nee (PTX_NEE_NO_LIGHT_SAMPLES gives this estimator) and its guides "
	                                    "with ptx_render_aov, or clear the motion (ptx_scene_set_motion(scene, NULL)) to render the scene as it stands");
}

namespace {
// One listed triangle as the light tree sees it (include/ptx.h: LIGHT PICK, THE TREE): the float64 centroid, the float32 box of the corners
// and the float64 power
struct LightLeaf {
	double centroid[3];
	float lo[3], hi[3];
	double power;
};
// The light tree of PTX_LIGHT_PICK_TREE over the list's entries, and each entry's path word. build_punctual_tree's rule with the centroid in
// the place of the position: FIFO splits by count along the widest axis of the centroids' bounds. A node's box holds the CORNERS below it.
void build_light_tree(const std::vector<LightLeaf>& leaves, std::vector<uint32_t>& nodes, std::vector<uint32_t>& path) {
	nodes.clear();
	path.assign(leaves.size(), 0u);
	if (leaves.empty()) return;
	auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
	struct Pending { uint32_t node, depth, word; std::vector<uint32_t> idx; };   // word: the steps from the root so far, bit i = step i went right
	std::deque<Pending> queue;
	std::vector<uint32_t> root(leaves.size());
	for (uint32_t k = 0; k < (uint32_t)leaves.size(); k++) root[k] = k;
	nodes.resize(8);
	queue.push_back(Pending{0u, 0u, 0u, std::move(root)});
	while (!queue.empty()) {
		Pending pd = std::move(queue.front());
		queue.pop_front();
		std::vector<uint32_t>& idx = pd.idx;
		float lo[3], hi[3];
		double clo[3], chi[3], power = 0;
		for (size_t i = 0; i < idx.size(); i++) {
			const LightLeaf& lf = leaves[idx[i]];
			for (int a = 0; a < 3; a++) {
				if (i == 0 || lf.lo[a] < lo[a]) lo[a] = lf.lo[a];
				if (i == 0 || lf.hi[a] > hi[a]) hi[a] = lf.hi[a];
				if (i == 0 || lf.centroid[a] < clo[a]) clo[a] = lf.centroid[a];
				if (i == 0 || lf.centroid[a] > chi[a]) chi[a] = lf.centroid[a];
			}
			power += lf.power;
		}
		uint32_t w7;
		if (idx.size() == 1) {
			w7 = 0x80000000u | idx[0];
			path[idx[0]] = pd.word;
		} else {
			int ax = 0;
			for (int a = 1; a < 3; a++)
				if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
			std::sort(idx.begin(), idx.end(), [&](uint32_t i, uint32_t j) {
				const double ci = leaves[i].centroid[ax], cj = leaves[j].centroid[ax];
				return ci < cj || (ci == cj && i < j);
			});
			const size_t half = idx.size() / 2;
			w7 = (uint32_t)(nodes.size() / 8);
			nodes.resize(nodes.size() + 16);
			const uint32_t bit = pd.depth < 32 ? 1u << pd.depth : 0u;   // a list the render accepts (<= 2^30 entries) is at most 31 steps deep
			queue.push_back(Pending{w7, pd.depth + 1, pd.word, std::vector<uint32_t>(idx.begin(), idx.begin() + half)});
			queue.push_back(Pending{w7 + 1, pd.depth + 1, pd.word | bit, std::vector<uint32_t>(idx.begin() + half, idx.end())});
		}
		uint32_t* q = nodes.data() + 8 * (size_t)pd.node;
		for (int a = 0; a < 3; a++) { q[a] = bits(lo[a]); q[4 + a] = bits(hi[a]); }
		q[3] = bits((float)power);
		q[7] = w7;
	}
}
}  // namespace

// The emissive triangles ptx_render_nee samples (include/ptx.h: the listing rules). World corners, areas and normals in float64 in the
// written order, stored as float32. In tree mode (ptx_scene_set_light_pick) the light tree and the path words are built with the list.
const ptx_scene::LightList* build_lights(ptx_scene* sc) {
	std::lock_guard<std::mutex> lk(sc->lights_mu);
	ptx_scene::LightList& ll = sc->lights;
	if (ll.built) return &ll;
	const FlatScene& h = sc->host;
	const size_t n_surf = h.surfaces.size();
	ll.surf_first.assign(n_surf, -1);
	std::vector<double> cum;
	double total = 0;
	const bool tree_mode = sc->light_pick == PTX_LIGHT_PICK_TREE;
	std::vector<LightLeaf> leaves;
	for (size_t s = 0; s < n_surf; s++) {
		const MaterialRec& m = h.materials[s];
		if (!(m.emissive[0] > 0 || m.emissive[1] > 0 || m.emissive[2] > 0)) continue;
		if (m.tex[2] >= 0 || !(m.opacity == 1.0f || std::fabs(m.opacity - 1.0f) < 0.0001f) || m.shadow_catcher) continue;   // can pass a sample through
		if (h.motion.set && h.motion.moved[h.surfaces[s].model]) continue;   // a moving model's emitter: unlisted, emission weight 1, no light samples
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
			if (tree_mode) {
				LightLeaf lf;
				for (int a = 0; a < 3; a++) {
					lf.centroid[a] = ((c[0][a] + c[1][a]) + c[2][a]) / 3.0;
					lf.lo[a] = (float)std::min(c[0][a], std::min(c[1][a], c[2][a]));
					lf.hi[a] = (float)std::max(c[0][a], std::max(c[1][a], c[2][a]));
				}
				lf.power = area * ((0.2126 * (double)m.emissive[0] + 0.7152 * (double)m.emissive[1]) + 0.0722 * (double)m.emissive[2]);
				leaves.push_back(lf);
			}
		}
	}
	for (double v : cum) ll.cdf.push_back((float)(v / total));
	if (!ll.cdf.empty()) ll.cdf.back() = 1.0f;
	ll.area = (float)total;
	if (tree_mode) build_light_tree(leaves, ll.tree, ll.path);
	ll.built = true;
	return &ll;
}

// The sampling table of the environment map (include/ptx.h: THE ENVIRONMENT TABLE). Luminances as the kernels' tex_pixel reads the texels,
// sums and shares in float64, stored as float32.
const ptx_scene::EnvTable* build_env_table(ptx_scene* sc) {
	std::lock_guard<std::mutex> lk(sc->lights_mu);
	ptx_scene::EnvTable& et = sc->env_table;
	if (et.built) return &et;
	et.built = true;
	const FlatScene& h = sc->host;
	if (h.env_tex < 0) return &et;
	const TexRec t = h.textures[(size_t)h.env_tex];
	const uint32_t w = t.w, hh = t.h, c = t.c_srgb & 255u;
	if (!w || !hh || !c) return &et;
	float lut[256];
	for (int b = 0; b < 256; b++) lut[b] = std::pow(b / 255.0F, 2.2F);
	auto chan = [&](uint32_t px, uint32_t py, uint32_t ch) -> double {   // tex_chan / tex_pixel: channels the image does not have are 1
		if (ch >= c) return 1.0;
		const bool srgb = (t.c_srgb & kTexSrgb) != 0 && ch < 3;
		const size_t at = (size_t)t.offset + ((size_t)py * w + px) * c + ch;
		if (t.c_srgb & kTexFloat) { const float v = h.texels_f[at]; return srgb ? std::pow(v, 2.2F) : v; }
		const uint32_t b = h.texels[at];
		return srgb ? lut[b] : (float)b / 255.0F;
	};
	std::vector<double> lum((size_t)w * hh);
	for (uint32_t j = 0; j < hh; j++)
		for (uint32_t i = 0; i < w; i++) {
			const double l = (0.2126 * chan(i, j, 0) + 0.7152 * chan(i, j, 1)) + 0.0722 * chan(i, j, 2);
			lum[(size_t)j * w + i] = l > 0 ? l : 0.0;   // negative and NaN count as 0
		}
	// weight = (luminance over the 3 x 3 texels the bilinear lookup can touch from inside the box, wrapped as tex_sample wraps) * cos(latitude of the row's centre)
	std::vector<double> wgt((size_t)w * hh), row_mass(hh);
	double total = 0;
	for (uint32_t j = 0; j < hh; j++) {
		const double lat = ((1.0 - ((double)j + 0.5) / (double)hh) - 0.5) / 0.3183;
		const double cl = std::max(std::cos(lat), 0.0);
		double mass = 0;
		for (uint32_t i = 0; i < w; i++) {
			double s = 0;
			for (int dj = -1; dj <= 1; dj++)
				for (int di = -1; di <= 1; di++) s += lum[(size_t)((j + hh + dj) % hh) * w + (i + w + di) % w];
			wgt[(size_t)j * w + i] = s * cl;
			mass += s * cl;
		}
		row_mass[j] = mass;
		total += mass;
	}
	if (!(total > 0) || !std::isfinite(total)) return &et;   // a black map: no table
	et.w = w; et.h = hh;
	et.row_cdf.resize(hh);
	et.cell_cdf.assign((size_t)w * hh, 0.0f);
	double cum = 0;
	for (uint32_t j = 0; j < hh; j++) {
		cum += row_mass[j];
		et.row_cdf[j] = (float)(cum / total);
		if (!(row_mass[j] > 0)) continue;   // a row of zero mass: all zeros
		double cc = 0;
		for (uint32_t i = 0; i < w; i++) {
			cc += wgt[(size_t)j * w + i];
			et.cell_cdf[(size_t)j * w + i] = (float)(cc / row_mass[j]);
		}
		et.cell_cdf[(size_t)j * w + w - 1] = 1.0f;
	}
	et.row_cdf[hh - 1] = 1.0f;
	return &et;
}

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
	c->queues.release(); c->spill.release(); c->sample_rad.release(); c->counters.release(); c->stage_a.release(); c->stage_b.release(); c->pixel_list.release(); c->srgb_thr.release(); c->round_ws.release(); c->denoise.release();
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
	{   // the sampling table belongs to the map that goes
		std::lock_guard<std::mutex> tl(sc->lights_mu);
		sc->env_table = ptx_scene::EnvTable{};
	}
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

// The light tree of PTX_PUNCTUAL_PICK_TREE over the stored records (include/ptx.h: PUNCTUAL PICK, THE TREE): [n_nodes][8] words. Nodes are
// split in FIFO order, by count along the widest axis; a black light is in no leaf. Empty without lights.
static std::vector<uint32_t> build_punctual_tree(const std::vector<float>& recs) {
	const uint32_t n = (uint32_t)(recs.size() / 16);
	std::vector<double> lum(n);
	std::vector<uint32_t> root;
	for (uint32_t k = 0; k < n; k++) {
		const float* r = recs.data() + 16 * (size_t)k;
		lum[k] = (0.2126 * (double)r[8] + 0.7152 * (double)r[9]) + 0.0722 * (double)r[10];
		if (lum[k] > 0) root.push_back(k);
	}
	std::vector<uint32_t> nodes;
	if (root.empty()) return nodes;
	auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
	std::deque<std::pair<uint32_t, std::vector<uint32_t>>> queue;   // (node, its lights in order)
	nodes.resize(8);
	queue.emplace_back(0u, std::move(root));
	while (!queue.empty()) {
		const uint32_t node = queue.front().first;
		std::vector<uint32_t> idx = std::move(queue.front().second);
		queue.pop_front();
		float lo[3], hi[3];
		double power = 0;
		for (size_t i = 0; i < idx.size(); i++) {
			const float* p = recs.data() + 16 * (size_t)idx[i];
			for (int a = 0; a < 3; a++) {
				if (i == 0 || p[a] < lo[a]) lo[a] = p[a];
				if (i == 0 || p[a] > hi[a]) hi[a] = p[a];
			}
			power += lum[idx[i]];
		}
		uint32_t w7;
		if (idx.size() == 1) {
			w7 = 0x80000000u | idx[0];
		} else {
			int ax = 0;
			for (int a = 1; a < 3; a++)
				if ((double)hi[a] - (double)lo[a] > (double)hi[ax] - (double)lo[ax]) ax = a;
			std::sort(idx.begin(), idx.end(), [&](uint32_t i, uint32_t j) {
				const float pi = recs[16 * (size_t)i + ax], pj = recs[16 * (size_t)j + ax];
				return pi < pj || (pi == pj && i < j);
			});
			const size_t half = idx.size() / 2;
			w7 = (uint32_t)(nodes.size() / 8);
			nodes.resize(nodes.size() + 16);
			queue.emplace_back(w7, std::vector<uint32_t>(idx.begin(), idx.begin() + half));
			queue.emplace_back(w7 + 1, std::vector<uint32_t>(idx.begin() + half, idx.end()));
		}
		uint32_t* q = nodes.data() + 8 * (size_t)node;
		for (int a = 0; a < 3; a++) { q[a] = bits(lo[a]); q[4 + a] = bits(hi[a]); }
		q[3] = bits((float)power);
		q[7] = w7;
	}
	return nodes;
}

int ptx_scene_set_punctual_pick(ptx_scene* sc, uint32_t pick) {
	// no device work: ptx_render_nee uploads the tree when it next runs
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_scene_set_punctual_pick: scene is NULL");
	if (pick != PTX_PUNCTUAL_PICK_CDF && pick != PTX_PUNCTUAL_PICK_TREE) return set_err(PTX_ERR_INVALID, "ptx_scene_set_punctual_pick: unknown mode");
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);   // no render of this scene is in flight
	std::lock_guard<std::mutex> tl(sc->lights_mu);
	if (pick == sc->punctual_pick) return PTX_OK;
	sc->punctual_pick = pick;
	sc->punctual.tree = pick == PTX_PUNCTUAL_PICK_TREE ? build_punctual_tree(sc->punctual.recs) : std::vector<uint32_t>();
	sc->punctual.on_device = false;
	return PTX_OK;
}

int ptx_scene_get_punctual_pick(const ptx_scene* sc, uint32_t* pick) {
	if (!sc || !pick) return set_err(PTX_ERR_INVALID, "ptx_scene_get_punctual_pick: NULL argument");
	std::lock_guard<std::mutex> tl(const_cast<ptx_scene*>(sc)->lights_mu);
	*pick = sc->punctual_pick;
	return PTX_OK;
}

int ptx_scene_set_light_pick(ptx_scene* sc, uint32_t pick) {
	// no device work: the list and the tree are rebuilt at the next request and uploaded by the next ptx_render_nee
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_scene_set_light_pick: scene is NULL");
	if (pick != PTX_LIGHT_PICK_CDF && pick != PTX_LIGHT_PICK_TREE) return set_err(PTX_ERR_INVALID, "ptx_scene_set_light_pick: unknown mode");
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);   // no render of this scene is in flight
	std::lock_guard<std::mutex> tl(sc->lights_mu);
	if (pick == sc->light_pick) return PTX_OK;
	sc->light_pick = pick;
	sc->lights = ptx_scene::LightList{};   // the tree lives and dies with the list: both are built anew, the list bit for bit as before
	return PTX_OK;
}

int ptx_scene_get_light_pick(const ptx_scene* sc, uint32_t* pick) {
	if (!sc || !pick) return set_err(PTX_ERR_INVALID, "ptx_scene_get_light_pick: NULL argument");
	std::lock_guard<std::mutex> tl(const_cast<ptx_scene*>(sc)->lights_mu);
	*pick = sc->light_pick;
	return PTX_OK;
}

int ptx_scene_set_punctual_lights(ptx_scene* sc, const float* lights, uint32_t n) {
	// every refusal is decided before any device work; the call itself does none (ptx_render_nee uploads the lights when it next runs)
	auto bad = [](const std::string& m) { return set_err(PTX_ERR_INVALID, "ptx_scene_set_punctual_lights: " + m); };
	if (!sc) return bad("scene is NULL");
	if (n && !lights) return bad("lights is NULL with n > 0");
	if (n > 65536u) return bad("more than 65536 lights");
	std::vector<double> cum(n);
	double total = 0;
	for (uint32_t k = 0; k < n; k++) {
		const float* r = lights + 16 * (size_t)k;
		const std::string at = "light " + std::to_string(k) + ": ";
		for (int a = 0; a < 16; a++)
			if (!std::isfinite(r[a])) return bad(at + "a field is not finite");
		if (r[7] != 0.0f && r[7] != 1.0f) return bad(at + "kind must be 0 (point) or 1 (spot)");
		if (r[8] < 0 || r[9] < 0 || r[10] < 0) return bad(at + "negative intensity");
		if (r[3] < 0) return bad(at + "negative range");
		if (r[7] == 1.0f) {
			const double len = std::sqrt(((double)r[4] * r[4] + (double)r[5] * r[5]) + (double)r[6] * r[6]);
			if (!(std::fabs(len - 1.0) <= 1e-3)) return bad(at + "a spot's direction must have unit length (within 1e-3)");
			if (r[11] < r[12]) return bad(at + "cos_inner < cos_outer");
		}
		total += (0.2126 * (double)r[8] + 0.7152 * (double)r[9]) + 0.0722 * (double)r[10];
		cum[k] = total;
	}
	ptx_scene::Punctual next;
	if (n && total > 0) {   // all lights black: no lights, as n = 0
		next.recs.assign(lights, lights + 16 * (size_t)n);
		next.cdf.resize(n);
		for (uint32_t k = 0; k < n; k++) next.cdf[k] = (float)(cum[k] / total);
		next.cdf[n - 1] = 1.0f;
	}
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);   // no render of this scene is in flight
	std::lock_guard<std::mutex> tl(sc->lights_mu);
	if (sc->punctual_pick == PTX_PUNCTUAL_PICK_TREE) next.tree = build_punctual_tree(next.recs);   // the mode outlives the lights
	sc->punctual = std::move(next);
	return PTX_OK;
}

int ptx_scene_set_camera(ptx_scene* sc, const ptx_camera* cam) {
	// every refusal is decided before any device work and before the scene is touched
	auto bad = [](const char* m) { return set_err(PTX_ERR_INVALID, std::string("ptx_scene_set_camera: ") + m); };
	if (!sc || !cam) return bad("NULL argument");
	for (int k = 0; k < 3; k++) if (!std::isfinite(cam->origin[k])) return bad("origin is not finite");
	for (int k = 0; k < 9; k++) if (!std::isfinite(cam->basis[k])) return bad("basis is not finite");
	if (!std::isfinite(cam->yfov) || !std::isfinite(cam->lens_radius) || !std::isfinite(cam->focus_distance) || !std::isfinite(cam->blade_rotation))
		return bad("a field is not finite");
	if (!(cam->yfov > 0) || !((double)cam->yfov < 3.14159265358979323846)) return bad("yfov must lie in (0, pi)");
	if (cam->lens_radius < 0) return bad("lens_radius < 0");
	if (cam->lens_radius > 0 && !(cam->focus_distance > 0)) return bad("a lens needs focus_distance > 0");
	if (cam->blades != 0 && (cam->blades < 3 || cam->blades > kLensMaxBlades)) return bad("blades must be 0 or 3 .. 32");
	CameraRec next{};
	memcpy(next.origin, cam->origin, 12);
	memcpy(next.basis, cam->basis, 36);
	next.fov = cam->yfov;
	next.tan_half_fov = std::tan(cam->yfov * 0.5F);   // as finalize_scene computes it
	if (cam->lens_radius > 0) {   // without a lens the lens fields are stored as zeros: the scene is the pinhole scene, whatever they held
		next.lens_radius = cam->lens_radius;
		next.focus_distance = cam->focus_distance;
		next.blades = cam->blades ? cam->blades : 16u;
		next.blade_rotation = cam->blade_rotation;
	}
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);   // no render of this scene is being queued
	if (sc->ctx && next.lens_radius > 0) {
		// the table goes into the scene's own buffer behind whatever is queued on the stream; nothing is freed or allocated. The source is
		// a local: the stream is synchronised before it goes
		ptx_ctx* c = sc->ctx;
		HIP_TRY(hipSetDevice(c->device));
		const std::vector<float> lens = lens_table(next);
		HIP_TRY(hipMemcpyAsync(sc->d_lens.p, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
	}
	sc->host.camera = next;
	if (sc->ctx) sc->dev.cam = next;   // a kernel argument: the next launch takes it
	if (drop_motion(sc) && sc->ctx) return upload_motion(sc);   // the camera's begin key no longer belongs to it: the motion ends (MOTION)
	return PTX_OK;
}

int ptx_scene_get_camera(const ptx_scene* sc, ptx_camera* out) {
	if (!sc || !out) return set_err(PTX_ERR_INVALID, "ptx_scene_get_camera: NULL argument");
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);
	const CameraRec& c = sc->host.camera;
	memcpy(out->origin, c.origin, 12);
	memcpy(out->basis, c.basis, 36);
	out->yfov = c.fov;
	out->lens_radius = c.lens_radius;
	out->focus_distance = c.focus_distance;
	out->blades = c.blades;
	out->blade_rotation = c.blade_rotation;
	return PTX_OK;
}

int ptx_scene_set_model_xforms(ptx_scene* sc, const float* model_xform, uint32_t n_models) {
	auto bad = [](const char* m) { return set_err(PTX_ERR_INVALID, std::string("ptx_scene_set_model_xforms: ") + m); };
	if (!sc || !model_xform) return bad("NULL argument");
	if ((size_t)n_models * 12 != sc->host.model_xform.size()) return bad("n_models differs from the scene's");   // the size never changes after creation
	for (size_t k = 0; k < (size_t)n_models * 12; k++)
		if (!std::isfinite(model_xform[k])) return bad("a value is not finite");
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);
	FlatScene& h = sc->host;
	h.model_xform.assign(model_xform, model_xform + (size_t)n_models * 12);
	h.motion = FlatScene::Motion{};   // the begin keys no longer belong to these transforms: the motion ends (MOTION)
	sc->dev_motion = DevMotion{};
	apply_model_xforms(h);   // model, space and shade records; no tree is built
	{   // world normals and areas of the emissive triangles moved with the models: the list is rebuilt at the next request
		std::lock_guard<std::mutex> tl(sc->lights_mu);
		sc->lights = ptx_scene::LightList{};
	}
	if (sc->ctx) return upload_scene(sc);   // every record goes up again, in stream order, into the buffers the scene already owns
	return PTX_OK;
}

int ptx_scene_set_motion(ptx_scene* sc, const ptx_motion* m) {
	// every refusal is decided before the scene is touched
	auto bad = [](const char* msg) { return set_err(PTX_ERR_INVALID, std::string("ptx_scene_set_motion: ") + msg); };
	if (!sc) return bad("NULL scene");
	const size_t n = sc->host.model_xform.size() / 12;
	if (m) {
		if (m->begin_model_xform && (size_t)m->n_models != n) return bad("n_models differs from the scene's");
		if (m->begin_model_xform)
			for (size_t k = 0; k < 12 * n; k++)
				if (!std::isfinite(m->begin_model_xform[k])) return bad("a begin transform value is not finite");
		if (const ptx_camera* cam = m->begin_camera) {   // what ptx_scene_set_camera refuses of origin, basis and yfov; the lens fields are ignored
			for (int k = 0; k < 3; k++) if (!std::isfinite(cam->origin[k])) return bad("begin camera: origin is not finite");
			for (int k = 0; k < 9; k++) if (!std::isfinite(cam->basis[k])) return bad("begin camera: basis is not finite");
			if (!std::isfinite(cam->yfov) || !(cam->yfov > 0) || !((double)cam->yfov < 3.14159265358979323846)) return bad("begin camera: yfov must lie in (0, pi)");
		}
		if (!(m->shutter_open >= 0.0f) || !(m->shutter_open <= m->shutter_close) || !(m->shutter_close <= 1.0f))
			return bad("the shutter must satisfy 0 <= open <= close <= 1");
	}
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);   // no render of this scene is being queued
	FlatScene& h = sc->host;
	const bool had_models = h.motion.set && h.motion.any_model();
	FlatScene::Motion next;
	if (m) {
		next.set = true;
		next.begin_xform = h.model_xform;   // a static model's begin key is its current transform, bit for bit
		next.moved.assign(n, 0u);
		if (m->begin_model_xform)
			for (size_t k = 0; k < n; k++)
				if (memcmp(m->begin_model_xform + 12 * k, h.model_xform.data() + 12 * k, 48)) {
					next.moved[k] = 1u;
					memcpy(next.begin_xform.data() + 12 * k, m->begin_model_xform + 12 * k, 48);
				}
		memcpy(next.begin_camera, h.camera.origin, 12);
		memcpy(next.begin_camera + 3, h.camera.basis, 36);
		if (m->begin_camera && (memcmp(m->begin_camera->origin, h.camera.origin, 12) || memcmp(m->begin_camera->basis, h.camera.basis, 36))) {
			next.camera_moved = true;
			memcpy(next.begin_camera, m->begin_camera->origin, 12);
			memcpy(next.begin_camera + 3, m->begin_camera->basis, 36);
		}
		next.shutter_open = m->shutter_open;
		next.shutter_close = m->shutter_close;
	}
	h.motion = std::move(next);
	if (had_models || h.motion.any_model()) {   // which models may share a ray space, and which emitters are listed, depend on who moves
		assign_ray_spaces(h);
		{
			std::lock_guard<std::mutex> tl(sc->lights_mu);
			sc->lights = ptx_scene::LightList{};
		}
		if (sc->ctx) return upload_motion(sc);
	}
	return PTX_OK;
}

int ptx_scene_motion_state(const ptx_scene* sc, float u, float* model_xform, float* camera) {
	if (!sc) return set_err(PTX_ERR_INVALID, "ptx_scene_motion_state: NULL scene");
	if (!std::isfinite(u)) return set_err(PTX_ERR_INVALID, "ptx_scene_motion_state: u is not finite");
	std::unique_lock<std::mutex> lk;
	if (sc->ctx) lk = std::unique_lock<std::mutex>(sc->ctx->mu);
	const FlatScene& h = sc->host;
	const FlatScene::Motion& mo = h.motion;
	const size_t n = h.model_xform.size() / 12;
	if (model_xform)
		for (size_t k = 0; k < n; k++) {
			if (mo.set && mo.moved[k]) motion_xform(mo.begin_xform.data() + 12 * k, h.model_xform.data() + 12 * k, u, model_xform + 12 * k);
			else memcpy(model_xform + 12 * k, h.model_xform.data() + 12 * k, 48);   // static: read without arithmetic
		}
	if (camera) {
		float cur[12];
		memcpy(cur, h.camera.origin, 12);
		memcpy(cur + 3, h.camera.basis, 36);
		if (mo.set && mo.camera_moved) motion_xform(mo.begin_camera, cur, u, camera);
		else memcpy(camera, cur, 48);
	}
	return PTX_OK;
}

int64_t ptx_gltf_read_punctual_lights(const char* gltf_path, float* dst, size_t dst_floats) {
	if (!gltf_path) return -(int64_t)set_err(PTX_ERR_INVALID, "ptx_gltf_read_punctual_lights: path is NULL");
	std::vector<float> recs;
	try {
		read_gltf_punctual_lights(gltf_path, recs);
	} catch (const Error& e) {
		return -(int64_t)set_err(e.code, e.msg);
	} catch (const std::exception& e) {
		return -(int64_t)set_err(PTX_ERR_PARSE, e.what());
	}
	if (dst) {
		if (dst_floats < recs.size()) return -(int64_t)set_err(PTX_ERR_INVALID, "ptx_gltf_read_punctual_lights: destination too small");
		if (!recs.empty()) memcpy(dst, recs.data(), recs.size() * 4);
	}
	return (int64_t)(recs.size() / 16);
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

int64_t ptx_scene_get_array(const ptx_scene* sc, ptx_array which, void* dst, size_t dst_bytes) {
	if (!sc) { set_err(PTX_ERR_INVALID, "scene is NULL"); return -1; }
	const FlatScene& h = sc->host;
	const void* src = nullptr;
	size_t bytes = 0, elem = 4;
	std::vector<float> tmp;
	std::vector<uint32_t> tmp_words;
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
	case PTX_ARR_LIGHT_TREE: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.tree.data(); bytes = ll.tree.size() * 4; break; }
	case PTX_ARR_LIGHT_PATH: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.path.data(); bytes = ll.path.size() * 4; break; }
	case PTX_ARR_LIGHT_GEOM: { const auto& ll = *build_lights(const_cast<ptx_scene*>(sc)); src = ll.geom.data(); bytes = ll.geom.size() * 4; break; }
	case PTX_ARR_ENV_ROW_CDF: { const auto& et = *build_env_table(const_cast<ptx_scene*>(sc)); src = et.row_cdf.data(); bytes = et.row_cdf.size() * 4; break; }
	case PTX_ARR_ENV_CELL_CDF: { const auto& et = *build_env_table(const_cast<ptx_scene*>(sc)); src = et.cell_cdf.data(); bytes = et.cell_cdf.size() * 4; break; }
	case PTX_ARR_PUNCTUAL: { std::lock_guard<std::mutex> tl(const_cast<ptx_scene*>(sc)->lights_mu); tmp = sc->punctual.recs; src = tmp.data(); bytes = tmp.size() * 4; break; }
	case PTX_ARR_PUNCTUAL_CDF: { std::lock_guard<std::mutex> tl(const_cast<ptx_scene*>(sc)->lights_mu); tmp = sc->punctual.cdf; src = tmp.data(); bytes = tmp.size() * 4; break; }
	case PTX_ARR_PUNCTUAL_TREE: { std::lock_guard<std::mutex> tl(const_cast<ptx_scene*>(sc)->lights_mu); tmp_words = sc->punctual.tree; src = tmp_words.data(); bytes = tmp_words.size() * 4; break; }
	case PTX_ARR_LENS: tmp = lens_table(h.camera); src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_TRI_ISECT: src = h.tri_isect.data(); bytes = h.tri_isect.size() * sizeof(TriIsect); break;
	case PTX_ARR_RES_NODES: src = h.res_nodes.data(); bytes = h.res_nodes.size() * 8; break;
	case PTX_ARR_RES_REFS: src = h.res_refs.data(); bytes = h.res_refs.size() * 4; break;
	case PTX_ARR_RES_TRIS: src = h.res_tris.data(); bytes = h.res_tris.size() * sizeof(TriIsect); break;
	case PTX_ARR_LDS_ROOT:     // the root and the layout bit, as before the shape bits existed; PTX_ARR_LDS_SHAPE: the whole word
	case PTX_ARR_LDS_SHAPE:
		for (auto& s : h.surfaces) {
			const uint32_t w = (which == PTX_ARR_LDS_SHAPE || s.lds_root == 0xFFFFFFFFu) ? s.lds_root : (s.lds_root & (kLdsRootMask | kLdsLeafOrderBit));
			float f; memcpy(&f, &w, 4); tmp.push_back(f);
		}
		src = tmp.data(); bytes = tmp.size() * 4; break;
	case PTX_ARR_MOTION_XFORM: if (h.motion.set) { src = h.motion.begin_xform.data(); bytes = h.motion.begin_xform.size() * 4; } break;
	case PTX_ARR_MOTION_MOVED: if (h.motion.set) { src = h.motion.moved.data(); bytes = h.motion.moved.size() * 4; } break;
	case PTX_ARR_MOTION_CAMERA:
		if (h.motion.set) {
			tmp.assign(h.motion.begin_camera, h.motion.begin_camera + 12);
			tmp.push_back(h.motion.camera_moved ? 1.0f : 0.0f); tmp.push_back(h.motion.shutter_open); tmp.push_back(h.motion.shutter_close);
			src = tmp.data(); bytes = tmp.size() * 4;
		}
		break;
	case PTX_ARR_SURF_AUX: src = h.surf_aux.data(); bytes = h.surf_aux.size() * sizeof(UnitAux); break;
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

}  // extern "C"
