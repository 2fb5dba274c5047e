// Stand-alone host check of plan_residency (scene_build.cpp): the LDS residency plan with ref-indexed and leaf-ordered surfaces, on the
// Cornell box and on a procedural scene, over a sweep of budgets. Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make -C distributed-path-tracer_amd/csrc plan_check`): the plan is plain index arithmetic over std::vectors, so the sanitizers see
// every read or write outside them. Usage: plan_residency_check <cornell.gltf>. Exit status 0 = every check held.
#include "../distributed-path-tracer_amd/csrc/flat_scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

using namespace ptx;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// One plan of `s` at `budget`: every resident leaf must name the records the full arrays name, whichever layout its surface got.
struct PlanFacts { std::vector<uint32_t> root; size_t n_marked = 0; };
static PlanFacts check_plan(FlatScene& s, size_t budget, bool leaf_order, const char* what) {
	plan_residency(s, budget, leaf_order);
	const size_t ns = s.surfaces.size();
	size_t n_res = 0, n_tris = 0, n_refs = 0, n_nodes = 0;
	int64_t spent = 0;
	PlanFacts f;
	for (size_t si = 0; si < ns; si++) {
		const uint32_t lr = s.surfaces[si].lds_root;
		f.root.push_back(lr);
		if (lr == 0xFFFFFFFFu) continue;
		n_res++;
		const bool lo = (lr & kLdsLeafOrderBit) != 0;
		CHECK(leaf_order || !lo, "%s: surface %zu leaf-ordered with the layout switched off", what, si);
		const int32_t* rg = &s.surf_range[8 * si];
		const uint32_t t0 = (uint32_t)rg[2], nt = (uint32_t)rg[3], node0 = (uint32_t)rg[4], nn = (uint32_t)rg[5], ref0 = (uint32_t)rg[6], nr = (uint32_t)rg[7];
		const uint32_t nb = (lr & kLdsRootMask) - (s.surfaces[si].kd_root - node0);
		CHECK((size_t)nb + nn <= s.res_nodes.size(), "%s: surface %zu: nodes [%u, +%u) of %zu", what, si, nb, nn, s.res_nodes.size());
		if ((size_t)nb + nn > s.res_nodes.size()) continue;
		n_nodes += nn; n_tris += lo ? nr : nt; n_refs += lo ? 0 : nr;
		if (lo) { f.n_marked++; const int64_t e = ((int64_t)nr - nt) * 48 - (int64_t)nr * 4; if (e > 0) spent += e; }
		for (uint32_t k = 0; k < nn; k++) {
			const KdNode full = s.kd_nodes[node0 + k], res = s.res_nodes[nb + k];
			if ((full.w1 & 3u) != KD_LEAF) {
				CHECK(res.w0 == full.w0 && (res.w1 & 15u) == (full.w1 & 15u) && (res.w1 >> 4) - nb == (full.w1 >> 4) - node0, "%s: surface %zu node %u: branch differs", what, si, k);
				continue;
			}
			const uint32_t count = full.w1 >> 2;
			CHECK(res.w1 == full.w1, "%s: surface %zu node %u: leaf count differs", what, si, k);
			CHECK(full.w0 >= ref0 && full.w0 + count <= ref0 + nr, "%s: surface %zu node %u: leaf outside the surface's references", what, si, k);
			for (uint32_t i = 0; i < count; i++) {
				size_t slot;
				if (lo) slot = (size_t)res.w0 + i;
				else {
					CHECK((size_t)res.w0 + i < s.res_refs.size(), "%s: surface %zu node %u: reference %u of %zu", what, si, k, res.w0 + i, s.res_refs.size());
					if ((size_t)res.w0 + i >= s.res_refs.size()) break;
					slot = s.res_refs[res.w0 + i];
				}
				CHECK(slot < s.res_tris.size(), "%s: surface %zu node %u: record %zu of %zu", what, si, k, slot, s.res_tris.size());
				if (slot >= s.res_tris.size()) break;
				const uint32_t gid = s.kd_refs[full.w0 + i];
				CHECK(gid >= t0 && gid < t0 + nt, "%s: surface %zu: reference to a foreign triangle", what, si);
				CHECK(!memcmp(&s.res_tris[slot], &s.tri_isect[gid], sizeof(TriIsect)), "%s: surface %zu node %u record %u: not triangle %u's", what, si, k, i, gid);
			}
		}
	}
	CHECK(n_res == s.n_resident, "%s: n_resident %u, counted %zu", what, s.n_resident, n_res);
	CHECK(n_tris == s.res_tris.size() && n_refs == s.res_refs.size() && n_nodes == s.res_nodes.size(), "%s: array sizes are not the sum of the regions", what);
	const size_t bytes = s.res_tris.size() * 48 + s.shade.size() * sizeof(ShadeRec) + pad16(s.res_nodes.size() * 8) + pad16(s.res_refs.size() * 4);
	CHECK(bytes == s.res_bytes, "%s: res_bytes %zu, regions %zu", what, s.res_bytes, bytes);
	CHECK(n_res == 0 || s.res_bytes <= budget, "%s: %zu bytes planned into a budget of %zu", what, s.res_bytes, budget);
	CHECK(spent <= (int64_t)kLdsLeafOrderCap, "%s: %lld bytes of extras, cap %zu", what, (long long)spent, kLdsLeafOrderCap);
	return f;
}

static void sweep(FlatScene& s, const char* name) {
	const size_t full = 160 * 1024;
	std::vector<size_t> budgets = {0, 1, 1000, full};
	for (size_t b = 1200; b < full; b += 1511) budgets.push_back(b);
	// around the point where everything is resident, byte by 16 bytes: the extras meet "what is left of the budget" there
	size_t all = s.shade.size() * sizeof(ShadeRec) + 48;
	for (size_t si = 0; si < s.surfaces.size(); si++) { const int32_t* rg = &s.surf_range[8 * si]; all += (size_t)rg[5] * 8 + (size_t)rg[7] * 4 + (size_t)rg[3] * 48; }
	for (size_t b = all > 256 ? all - 256 : 0; b < all + 6000 && b <= full; b += 16) budgets.push_back(b);
	size_t max_marked = 0;
	for (size_t b : budgets) {
		char what[128];
		snprintf(what, sizeof what, "%s budget %zu refs", name, b);
		const PlanFacts off = check_plan(s, b, false, what);
		snprintf(what, sizeof what, "%s budget %zu leaf order", name, b);
		const PlanFacts on = check_plan(s, b, true, what);
		for (size_t si = 0; si < off.root.size(); si++)
			CHECK((off.root[si] == 0xFFFFFFFFu) == (on.root[si] == 0xFFFFFFFFu), "%s: residency of surface %zu depends on the layout", what, si);
		CHECK(off.n_marked == 0, "%s: marked surfaces with the layout off", what);
		max_marked = std::max(max_marked, on.n_marked);
	}
	printf("%s: %zu surfaces, %zu budgets, at most %zu leaf-ordered\n", name, s.surfaces.size(), budgets.size(), max_marked);
	CHECK(max_marked > 0, "%s: no surface was ever leaf-ordered", name);
}

// A procedural scene from arrays: quads of 2 triangles (leaves that share nothing), a fan whose triangles overlap heavily (leaves share
// many) and a tessellated bumpy grid (a deep tree), in two models.
static void procedural(FlatScene& s) {
	auto vert = [&](float x, float y, float z) { const float v[11] = {x, y, z, 0, 0, 0, 1, 0, 1, 0, 0}; s.vertices.insert(s.vertices.end(), v, v + 11); };
	auto begin = [&]() { const int32_t rg[8] = {(int32_t)(s.vertices.size() / 11), 0, (int32_t)(s.triangles.size() / 3), 0, 0, 0, 0, 0}; s.surf_range.insert(s.surf_range.end(), rg, rg + 8); };
	auto end = [&]() {
		int32_t* rg = &s.surf_range[s.surf_range.size() - 8];
		rg[1] = (int32_t)(s.vertices.size() / 11) - rg[0]; rg[3] = (int32_t)(s.triangles.size() / 3) - rg[2];
		const float m[11] = {0.8f, 0.8f, 0.8f, 1, 0.5f, 0, 0, 0, 0, 1.5f, 0};
		s.materials_raw.insert(s.materials_raw.end(), m, m + 11);
		s.material_tex.insert(s.material_tex.end(), 7, 0);
	};
	auto tri = [&](uint32_t a, uint32_t b, uint32_t c) { s.triangles.push_back(a); s.triangles.push_back(b); s.triangles.push_back(c); };
	for (int q = 0; q < 3; q++) {   // quads
		begin();
		vert(-1, (float)q, -1); vert(1, (float)q, -1); vert(1, (float)q, 1); vert(-1, (float)q, 1);
		tri(0, 1, 2); tri(0, 2, 3);
		end();
	}
	begin();   // fan: 24 long slivers around one corner
	vert(0, 0, 0);
	for (int k = 0; k <= 24; k++) vert(4 * std::cos(0.06f * k), 0.3f * std::sin(1.7f * k), 4 * std::sin(0.06f * k));
	for (uint32_t k = 0; k < 24; k++) tri(0, 1 + k, 2 + k);
	end();
	begin();   // grid 24 x 24 cells
	const int G = 24;
	for (int j = 0; j <= G; j++) for (int i = 0; i <= G; i++) vert(i * 0.25f, 0.2f * std::sin(0.9f * i) * std::cos(0.7f * j), j * 0.25f);
	for (uint32_t j = 0; j < (uint32_t)G; j++) for (uint32_t i = 0; i < (uint32_t)G; i++) {
		const uint32_t a = j * (G + 1) + i;
		tri(a, a + 1, a + G + 2); tri(a, a + G + 2, a + G + 1);
	}
	end();
	const float x0[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, x1[12] = {2, 1, -3, 0, 0, 2, 0, 2, 0, -2, 0, 0};
	s.model_xform.insert(s.model_xform.end(), x0, x0 + 12); s.model_xform.insert(s.model_xform.end(), x1, x1 + 12);
	const int32_t ms[4] = {0, 3, 3, 2};
	s.model_surf.assign(ms, ms + 4);
	s.model_names = {"quads", "fan and grid"};
	const float cam[13] = {0, 1, 8, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.8f};
	finalize_scene(s, cam, nullptr);
}

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s <cornell.gltf>\n", argv[0]); return 2; }
	try {
		FlatScene cornell;
		load_gltf(argv[1], 0u, 0u, WorkFilter{}, cornell);
		sweep(cornell, "cornell");
		// the default plan of the Cornell box: the two boxes, the three wall surfaces and the light leaf-ordered, the sphere behind references
		check_plan(cornell, 160 * 1024, true, "cornell default");
		size_t big = 0;
		for (size_t si = 0; si < cornell.surfaces.size(); si++) if (cornell.surf_range[8 * si + 3] > cornell.surf_range[8 * big + 3]) big = si;
		for (size_t si = 0; si < cornell.surfaces.size(); si++) {
			const uint32_t lr = cornell.surfaces[si].lds_root;
			CHECK(lr != 0xFFFFFFFFu && ((lr & kLdsLeafOrderBit) != 0) == (si != big), "cornell default: surface %zu root %08x", si, lr);
		}
		FlatScene proc;
		procedural(proc);
		sweep(proc, "procedural");
		// moving the models (ptx_scene_set_model_xforms' host part): the records are those of a scene finalized with the moved transforms,
		// the residency plan still holds, and moving back restores the first records; the aperture table of every blade count
		FlatScene moved;
		procedural(moved);
		const std::vector<ModelRec> first = moved.models;
		std::swap_ranges(moved.model_xform.begin(), moved.model_xform.begin() + 12, moved.model_xform.begin() + 12);
		apply_model_xforms(moved);
		FlatScene fresh;
		procedural(fresh);   // procedural() finalizes with its own transforms: swap them and redo the tail on a second scene
		fresh.model_xform = moved.model_xform;
		apply_model_xforms(fresh);
		CHECK(moved.models.size() == fresh.models.size() && !memcmp(moved.models.data(), fresh.models.data(), moved.models.size() * sizeof(ModelRec)), "moved model records");
		CHECK(moved.shade.size() == fresh.shade.size() && !memcmp(moved.shade.data(), fresh.shade.data(), moved.shade.size() * sizeof(ShadeRec)), "moved shade records");
		CHECK(moved.spaces.size() == 2 && moved.model_space.size() == 2, "moved ray spaces: %zu", moved.spaces.size());
		sweep(moved, "procedural, models moved");
		std::swap_ranges(moved.model_xform.begin(), moved.model_xform.begin() + 12, moved.model_xform.begin() + 12);
		apply_model_xforms(moved);
		CHECK(!memcmp(moved.models.data(), first.data(), first.size() * sizeof(ModelRec)), "models moved back");
		for (uint32_t n = 3; n <= kLensMaxBlades; n++) {
			CameraRec cam{};
			cam.lens_radius = 0.5f; cam.focus_distance = 2; cam.blades = n; cam.blade_rotation = 0.1f * n;
			const std::vector<float> t = lens_table(cam);
			CHECK(t.size() == 2 * (size_t)(n + 1) && !memcmp(&t[0], &t[2 * n], 8), "aperture table of %u blades", n);
			for (uint32_t k = 0; k < n; k++) CHECK(std::fabs(std::hypot(t[2 * k], t[2 * k + 1]) - 0.5f) < 1e-6f, "corner %u of %u", k, n);
		}
		CHECK(lens_table(CameraRec{}).empty(), "no table without a lens");
	} catch (const Error& e) {
		fprintf(stderr, "error %d: %s\n", e.code, e.msg.c_str());
		return 2;
	}
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("plan_residency_check: ok\n");
	return 0;
}
