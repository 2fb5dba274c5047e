// Stand-alone host check of kd_chain_shape and of the chain flag plan_residency puts into the auxiliary surface table (kAuxChainBit,
// flat_scene.hpp): on the Cornell box and on the small quads of tests/test_kd_chain.py, the flag is compared with a brute-force reading of
// the full node array. Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make -C distributed-path-tracer_amd/csrc chain_check`). Usage: kd_chain_check <cornell.gltf>. Exit status 0 = every check held.
#include "../distributed-path-tracer_amd/csrc/flat_scene.hpp"

#include <cstdio>
#include <cstring>

using namespace ptx;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

// branch levels of the chain at `n` of the full node array, -1 when some node has both children or none; `right`: a branch keeps its right child
static int brute_chain(const std::vector<KdNode>& nodes, uint32_t n, bool* right = nullptr) {
	int levels = 0;
	for (;;) {
		const uint32_t w1 = nodes.at(n).w1;
		if ((w1 & 3u) == KD_LEAF) return levels;
		const bool hl = w1 & 4u, hr = w1 & 8u;
		if (hl == hr) return -1;
		if (right && hr) *right = true;
		levels++;
		n = w1 >> 4;
	}
}

// The plan at `budget` under the settings: the flag is the brute-force one exactly on the resident, leaf-ordered surfaces, absent elsewhere
// and with the switch off, and the resident copy the kernels walk is the chain the full tree is.
static void check_plan(FlatScene& s, size_t budget, const char* what) {
	plan_residency(s, budget, true, false);
	for (size_t si = 0; si < s.surfaces.size(); si++) CHECK((s.surf_aux.at(si).flags & kAuxChainBit) == 0, "%s: surface %zu: flag with the switch off", what, si);
	plan_residency(s, budget, false, true);
	for (size_t si = 0; si < s.surfaces.size(); si++) CHECK((s.surf_aux.at(si).flags & kAuxChainBit) == 0, "%s: surface %zu: flag on a ref-indexed surface", what, si);
	plan_residency(s, budget, true, true);
	CHECK(s.surf_aux.size() == s.surfaces.size(), "%s: table size", what);
	for (size_t si = 0; si < s.surfaces.size(); si++) {
		const uint32_t lr = s.surfaces[si].lds_root;
		const int levels = brute_chain(s.kd_nodes, s.surfaces[si].kd_root);
		const bool want = lr != 0xFFFFFFFFu && (lr & kLdsLeafOrderBit) && levels >= 0;
		CHECK(((s.surf_aux[si].flags & kAuxChainBit) != 0) == want, "%s: surface %zu: flag %u, brute force %d levels, lds_root %08x", what, si, s.surf_aux[si].flags, levels, lr);
		CHECK(kd_chain_shape(s.kd_nodes, s.surfaces[si].kd_root) == levels, "%s: surface %zu: kd_chain_shape on the full tree", what, si);
		if (lr != 0xFFFFFFFFu) CHECK(kd_chain_shape(s.res_nodes, lr & kLdsRootMask) == levels, "%s: surface %zu: resident copy", what, si);
		if (want && levels == 0) CHECK((lr & kLdsLeafOnlyBit) != 0, "%s: surface %zu: a chain of zero levels without the leaf-only bit", what, si);
	}
}

struct Quad { float p[4][3]; int levels; };
// tests/test_kd_chain.py: QUADS
static const Quad kQuads[] = {{{{-1, 0, 0}, {-1, 2, 0}, {-1, 2, 3}, {-1, 0, 3}}, 1},
                              {{{0, -2, 0}, {0, -2, 3}, {2, -2, 3}, {2, -2, 0}}, 1},
                              {{{0, 0, -1.5f}, {2, 0, -1.5f}, {2, 3, -1.5f}, {0, 3, -1.5f}}, 1},
                              {{{-3, -3, 1}, {-1, -3, 1}, {-1, -1, 2}, {-3, -1, 2}}, 2},
                              {{{-3, -3, -3}, {-1, -3, -2.5f}, {-1, -1, -1}, {-3, -1, -1.5f}}, 3},
                              {{{1, 0, 0}, {1, 2, 0}, {1, 2, 3}, {1, 0, 3}}, 0},
                              {{{0.5f, 1, 0.5f}, {2.5f, 1, 0.5f}, {2.5f, 1.5f, 2.5f}, {0.5f, 1.5f, 2.5f}}, 0}};

static void build_quads(FlatScene& s) {
	for (const Quad& q : kQuads) {
		const int32_t v0 = (int32_t)(s.vertices.size() / 11), t0 = (int32_t)(s.triangles.size() / 3);
		for (int k = 0; k < 4; k++) { const float v[11] = {q.p[k][0], q.p[k][1], q.p[k][2], 0, 0, 0, 1, 0, 1, 0, 0}; s.vertices.insert(s.vertices.end(), v, v + 11); }
		const uint32_t t[6] = {0, 2, 1, 0, 3, 2};
		s.triangles.insert(s.triangles.end(), t, t + 6);
		const int32_t rg[8] = {v0, 4, t0, 2, 0, 0, 0, 0};
		s.surf_range.insert(s.surf_range.end(), rg, rg + 8);
		const float mat[11] = {0.8f, 0.8f, 0.8f, 1, 0.5f, 0, 0, 0, 0, 1.5f, 0};
		s.materials_raw.insert(s.materials_raw.end(), mat, mat + 11);
		s.material_tex.insert(s.material_tex.end(), 7, 0);
	}
	const float x0[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
	s.model_xform.assign(x0, x0 + 12);
	const int32_t ms[2] = {0, (int32_t)(sizeof kQuads / sizeof kQuads[0])};
	s.model_surf.assign(ms, ms + 2);
	s.model_names = {"quads"};
	const float cam[13] = {0, 0, 10, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5f};
	finalize_scene(s, cam, nullptr);
}

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s <cornell.gltf>\n", argv[0]); return 2; }
	try {
		FlatScene cornell;
		load_gltf(argv[1], 0u, 0u, WorkFilter{}, cornell);
		const size_t full = 160 * 1024;
		for (size_t b = 0; b <= full; b += 4099) check_plan(cornell, b, "cornell sweep");
		check_plan(cornell, full, "cornell");
		// the default plan: the boxes and the green wall single leaves, the red wall one left-only branch above a leaf, the rest no chains
		const int want[7] = {0, 0, -1, 1, 0, -1, -1};
		CHECK(cornell.surfaces.size() == 7, "cornell: %zu surfaces", cornell.surfaces.size());
		for (size_t si = 0; si < cornell.surfaces.size() && si < 7; si++) {
			const int lv = brute_chain(cornell.kd_nodes, cornell.surfaces[si].kd_root);
			CHECK(lv == want[si], "cornell: surface %zu: %d levels, expected %d", si, lv, want[si]);
			CHECK(((cornell.surf_aux[si].flags & kAuxChainBit) != 0) == (want[si] >= 0 && si != 6), "cornell: surface %zu: flags %u", si, cornell.surf_aux[si].flags);
		}
		FlatScene q;
		build_quads(q);
		check_plan(q, full, "quads");
		check_plan(q, 2000, "quads, some not resident");
		bool right = false;
		for (size_t si = 0; si < q.surfaces.size(); si++) {
			const int lv = brute_chain(q.kd_nodes, q.surfaces[si].kd_root, &right);
			CHECK(lv == kQuads[si].levels, "quads: surface %zu: %d levels, expected %d", si, lv, kQuads[si].levels);
		}
		CHECK(!right, "a right-only branch: the reference's builder was not expected to make one (tests/test_kd_chain.py)");
		// kd_chain_shape refuses indices outside the array, both-children and childless branches, and a cycle
		CHECK(kd_chain_shape(q.res_nodes, (uint32_t)q.res_nodes.size()) == -1 && kd_chain_shape({}, 0) == -1, "root outside the array");
		CHECK(kd_chain_shape({kd_make_branch(0.5f, 0, true, false, 7)}, 0) == -1, "child outside the array");
		CHECK(kd_chain_shape({kd_make_branch(0.5f, 0, true, true, 1), kd_make_leaf(0, 0), kd_make_leaf(0, 0)}, 0) == -1, "both children");
		CHECK(kd_chain_shape({kd_make_branch(0.5f, 0, false, false, 1), kd_make_leaf(0, 0)}, 0) == -1, "no child");
		CHECK(kd_chain_shape({kd_make_branch(0.5f, 0, false, true, 0)}, 0) == -1, "a branch that is its own child");
		CHECK(kd_chain_shape({kd_make_branch(0.5f, 1, false, true, 1), kd_make_branch(0.25f, 2, true, false, 2), kd_make_leaf(0, 1)}, 0) == 2, "a hand-made right-then-left chain");
	} catch (const Error& e) {
		fprintf(stderr, "error %d: %s\n", e.code, e.msg.c_str());
		return 1;
	}
	if (g_fail) { fprintf(stderr, "kd_chain_check: %d check(s) failed\n", g_fail); return 1; }
	printf("kd_chain_check: ok\n");
	return 0;
}
