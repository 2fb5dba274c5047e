// Stand-alone host check of the shape bits plan_residency puts into SurfaceRec::lds_root (kLdsLeafOnlyBit / kLdsCompleteBit, flat_scene.hpp):
// on the Cornell box and on a boundary set of small procedural meshes, the bits are compared with a brute-force recomputation from the node
// arrays (the full ones, not the resident copy the plan read). Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make -C distributed-path-tracer_amd/csrc shapes_check`). Usage: kd_shapes_check <cornell.gltf> [explore]. Exit status 0 = every check held.
// `explore` prints the shape of a range of meshes instead: how the boundary set below (and tests/test_kd_shapes.py's copy of it) was chosen.
#include "../distributed-path-tracer_amd/csrc/flat_scene.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

using namespace ptx;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

// What the walk of the tree at `n` needs, by plain recursion over the full node array: does every branch have both children, and how many
// branch nodes does the longest root-to-leaf path hold
struct Facts { bool complete; int levels; };
static Facts facts(const std::vector<KdNode>& nodes, uint32_t n) {
	const uint32_t w1 = nodes.at(n).w1;
	if ((w1 & 3u) == KD_LEAF) return {true, 0};
	const bool hl = w1 & 4u, hr = w1 & 8u;
	Facts f{hl && hr, 0};
	const uint32_t li = w1 >> 4, ri = li + (hl ? 1u : 0u);
	if (hl) { const Facts a = facts(nodes, li); f.complete = f.complete && a.complete; f.levels = std::max(f.levels, a.levels); }
	if (hr) { const Facts b = facts(nodes, ri); f.complete = f.complete && b.complete; f.levels = std::max(f.levels, b.levels); }
	f.levels += 1;
	return f;
}
static uint32_t brute_shape(const FlatScene& s, size_t si) {
	const uint32_t root = s.surfaces[si].kd_root;
	if ((s.kd_nodes.at(root).w1 & 3u) == KD_LEAF) return kLdsLeafOnlyBit;
	const Facts f = facts(s.kd_nodes, root);
	return (f.complete && f.levels <= kShapeMaxBranchLevels) ? kLdsCompleteBit : 0u;
}

// The plan at `budget` under the three settings: the bits are the brute-force ones exactly on the leaf-ordered surfaces, absent elsewhere
// and with the switch off, and they change nothing else of the plan.
static void check_plan(FlatScene& s, size_t budget, const char* what) {
	plan_residency(s, budget, true, false);
	std::vector<uint32_t> off;
	for (const SurfaceRec& sr : s.surfaces) off.push_back(sr.lds_root);
	const std::vector<KdNode> nodes_off = s.res_nodes;
	const size_t bytes_off = s.res_bytes;
	plan_residency(s, budget, true, true);
	CHECK(s.res_bytes == bytes_off && s.res_nodes.size() == nodes_off.size() && (nodes_off.empty() || !memcmp(s.res_nodes.data(), nodes_off.data(), nodes_off.size() * sizeof(KdNode))),
	      "%s: the resident arrays depend on the shape switch", what);
	for (size_t si = 0; si < s.surfaces.size(); si++) {
		const uint32_t lr = s.surfaces[si].lds_root;
		CHECK((off[si] & (kLdsLeafOnlyBit | kLdsCompleteBit)) == 0 || off[si] == 0xFFFFFFFFu, "%s: surface %zu: shape bits with the switch off (%08x)", what, si, off[si]);
		if (lr == 0xFFFFFFFFu) { CHECK(off[si] == 0xFFFFFFFFu, "%s: surface %zu: residency depends on the shape switch", what, si); continue; }
		CHECK((lr & ~(kLdsLeafOnlyBit | kLdsCompleteBit)) == off[si], "%s: surface %zu: root or layout bit differ (%08x, %08x)", what, si, lr, off[si]);
		const uint32_t want = (lr & kLdsLeafOrderBit) ? brute_shape(s, si) : 0u;
		CHECK((lr & (kLdsLeafOnlyBit | kLdsCompleteBit)) == want, "%s: surface %zu: shape bits %08x, brute force %08x", what, si, lr & (kLdsLeafOnlyBit | kLdsCompleteBit), want);
		CHECK((lr & kLdsRootMask) < s.res_nodes.size(), "%s: surface %zu: root %u of %zu", what, si, lr & kLdsRootMask, s.res_nodes.size());
		// the copy the kernels walk has the shape the full tree has
		if ((lr & kLdsRootMask) < s.res_nodes.size()) CHECK(kd_tree_shape(s.res_nodes, lr & kLdsRootMask) == brute_shape(s, si), "%s: surface %zu: resident copy", what, si);
	}
	plan_residency(s, budget, false, true);
	for (size_t si = 0; si < s.surfaces.size(); si++)
		CHECK(s.surfaces[si].lds_root == 0xFFFFFFFFu || (s.surfaces[si].lds_root & ~kLdsRootMask) == 0, "%s: surface %zu: bits on a ref-indexed surface", what, si);
	plan_residency(s, budget, true, true);
}

// ---- the boundary meshes: nx x nz quads of side 0.5 in the plane y = `y`; L: the quarter i >= nx / 2, j >= nz / 2 left out;
// FIN: one more quad standing 2 above the grid's first cell; ZIG: the quads of a strip (nx = 1) rise and fall by 0.5 in turn along z, so that
// the box has the same extent on all axes as every leaf's (a tree whose walks set entries aside: a flat grid's box is 2e-4 thick and its
// split distances hardly ever fall inside a ray's interval). tests/test_kd_shapes.py builds the same arrays.
enum Kind { FLAT = 0, L = 1, FIN = 2, ZIG = 3 };
struct MeshSpec { int nx, nz; Kind kind; };
static void add_mesh(FlatScene& s, const MeshSpec& m, float y) {
	const int32_t v0 = (int32_t)(s.vertices.size() / 11), t0 = (int32_t)(s.triangles.size() / 3);
	auto vert = [&](float x, float yy, float z) { const float v[11] = {x, yy, z, 0, 0, 0, 1, 0, 1, 0, 0}; s.vertices.insert(s.vertices.end(), v, v + 11); };
	auto quad = [&](float x0, float y0, float z0, float x1, float y1, float z1) {   // (x0, y0, z0) - (x1, y0, z0) - (x1, y1, z1) - (x0, y1, z1)
		const uint32_t b = (uint32_t)(s.vertices.size() / 11) - (uint32_t)v0;
		vert(x0, y0, z0); vert(x1, y0, z0); vert(x1, y1, z1); vert(x0, y1, z1);
		const uint32_t t[6] = {b, b + 2, b + 1, b, b + 3, b + 2};
		s.triangles.insert(s.triangles.end(), t, t + 6);
	};
	for (int i = 0; i < m.nx; i++)
		for (int j = 0; j < m.nz; j++) {
			if (m.kind == L && i >= m.nx / 2 && j >= m.nz / 2) continue;
			if (m.kind == ZIG) quad(0.5f * i, y + (j % 2 ? 0.5f : 0.0f), 0.5f * j, 0.5f * (i + 1), y + (j % 2 ? 0.0f : 0.5f), 0.5f * (j + 1));
			else quad(0.5f * i, y, 0.5f * j, 0.5f * (i + 1), y, 0.5f * (j + 1));
		}
	if (m.kind == FIN) quad(0.0f, y + 2.0f, 0.0f, 0.5f, y + 2.0f, 0.5f);
	const int32_t rg[8] = {v0, (int32_t)(s.vertices.size() / 11) - v0, t0, (int32_t)(s.triangles.size() / 3) - t0, 0, 0, 0, 0};
	s.surf_range.insert(s.surf_range.end(), rg, rg + 8);
	const float mat[11] = {0.8f, 0.8f, 0.8f, 1, 0.5f, 0, 0, 0, 0, 1.5f, 0};
	s.materials_raw.insert(s.materials_raw.end(), mat, mat + 11);
	s.material_tex.insert(s.material_tex.end(), 7, 0);
}
static void build(FlatScene& s, const std::vector<MeshSpec>& meshes) {
	for (size_t k = 0; k < meshes.size(); k++) add_mesh(s, meshes[k], 4.0f * (float)k);
	const float x0[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
	s.model_xform.assign(x0, x0 + 12);
	const int32_t ms[2] = {0, (int32_t)meshes.size()};
	s.model_surf.assign(ms, ms + 2);
	s.model_names = {"boundary"};
	const float cam[13] = {1, 40, 1, 1, 0, 0, 0, 0, -1, 0, 1, 0, 0.8f};
	finalize_scene(s, cam, nullptr);
}
static const char* name_of(const FlatScene& s, size_t si, int* levels = nullptr, bool* complete = nullptr) {
	const Facts f = facts(s.kd_nodes, s.surfaces[si].kd_root);
	if (levels) *levels = f.levels;
	if (complete) *complete = f.complete;
	const uint32_t b = brute_shape(s, si);
	return b == kLdsLeafOnlyBit ? "LEAF_ONLY" : b == kLdsCompleteBit ? "COMPLETE_SHALLOW" : "general";
}

// The boundary set (chosen with `explore`): a single leaf; complete trees of 2, 3 (twice: 9 and 15 nodes), 4 (17 nodes twice, one of them
// from a square grid) and 6 branch levels; a branch with one child at 2 branch levels and one at 4; two zigzag strips, whose boxes have
// volume: a complete tree of 3 branch levels (13 nodes) and one of 4. main checks the four classes.
static const std::vector<MeshSpec> kBoundary = {{1, 1, FLAT}, {1, 2, FLAT}, {1, 4, FLAT}, {1, 7, FLAT}, {1, 8, FLAT}, {2, 2, FLAT}, {1, 1, FIN}, {2, 2, L}, {4, 4, FLAT},
                                                {1, 7, ZIG}, {1, 8, ZIG}};

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s <cornell.gltf> [explore]\n", argv[0]); return 2; }
	try {
		if (argc > 2 && !strcmp(argv[2], "explore")) {
			for (int kind = 0; kind < 4; kind++)
				for (int nx = 1; nx <= 8; nx++)
					for (int nz = nx; nz <= 8; nz++) {
						if ((kind == L && nx < 2) || (kind == ZIG && nx > 1)) continue;   // nothing would be left of the grid; a strip
						FlatScene s;
						build(s, {{nx, nz, (Kind)kind}});
						int lv; bool cp;
						const char* n = name_of(s, 0, &lv, &cp);
						printf("kind %d %d x %d: %3d tris %3d nodes  branch levels %d  %s  -> %s\n", kind, nx, nz, s.surf_range[3], s.surf_range[5], lv, cp ? "complete" : "missing child", n);
					}
			return 0;
		}
		FlatScene cornell;
		load_gltf(argv[1], 0u, 0u, WorkFilter{}, cornell);
		const size_t full = 160 * 1024;
		for (size_t b = 0; b <= full; b += 4099) check_plan(cornell, b, "cornell sweep");
		check_plan(cornell, full, "cornell");
		// the Cornell box as the default plan holds it: the white walls and the light complete and shallow, the boxes and the green wall a
		// single leaf, the red wall (an empty-space cut: a branch with one child) and the sphere (thousands of nodes, ref-indexed) general
		const uint32_t want[7] = {kLdsLeafOnlyBit, kLdsLeafOnlyBit, kLdsCompleteBit, 0u, kLdsLeafOnlyBit, kLdsCompleteBit, 0u};
		CHECK(cornell.surfaces.size() == 7, "cornell: %zu surfaces", cornell.surfaces.size());
		for (size_t si = 0; si < cornell.surfaces.size() && si < 7; si++) {
			const uint32_t lr = cornell.surfaces[si].lds_root;
			CHECK(lr != 0xFFFFFFFFu && (lr & (kLdsLeafOnlyBit | kLdsCompleteBit)) == want[si], "cornell: surface %zu lds_root %08x, expected shape %08x", si, lr, want[si]);
			printf("cornell surface %zu: %s\n", si, name_of(cornell, si));
		}
		FlatScene bd;
		build(bd, kBoundary);
		for (size_t b = 0; b <= full; b += 1511) check_plan(bd, b, "boundary sweep");
		check_plan(bd, full, "boundary");
		bool at_limit = false, one_more = false, shallow_missing = false, leaf_only = false;
		for (size_t si = 0; si < bd.surfaces.size(); si++) {
			int lv; bool cp;
			const char* n = name_of(bd, si, &lv, &cp);
			const uint32_t lr = bd.surfaces[si].lds_root;
			printf("boundary surface %zu (%d x %d, kind %d): branch levels %d, %s -> %s, lds_root %08x\n", si, kBoundary[si].nx, kBoundary[si].nz, (int)kBoundary[si].kind, lv, cp ? "complete" : "missing child", n, lr);
			CHECK(lr != 0xFFFFFFFFu, "boundary: surface %zu is not resident", si);
			if (lr == 0xFFFFFFFFu || !(lr & kLdsLeafOrderBit)) continue;   // a class counts only where the layout would have allowed a shape bit
			const uint32_t bits = lr & (kLdsLeafOnlyBit | kLdsCompleteBit);
			at_limit |= cp && lv == kShapeMaxBranchLevels && bits == kLdsCompleteBit;
			one_more |= cp && lv == kShapeMaxBranchLevels + 1 && bits == 0u;
			shallow_missing |= !cp && lv >= 1 && lv <= kShapeMaxBranchLevels && bits == 0u;
			leaf_only |= lv == 0 && bits == kLdsLeafOnlyBit;
		}
		CHECK(at_limit, "boundary: no complete tree at exactly %d branch levels that qualifies", kShapeMaxBranchLevels);
		CHECK(one_more, "boundary: no complete tree of %d branch levels that does not qualify", kShapeMaxBranchLevels + 1);
		CHECK(shallow_missing, "boundary: no shallow tree with a missing child");
		CHECK(leaf_only, "boundary: no leaf-only tree");
		// kd_tree_shape refuses indices outside the array instead of reading there
		CHECK(kd_tree_shape(bd.res_nodes, (uint32_t)bd.res_nodes.size()) == 0u && kd_tree_shape({}, 0) == 0u, "root outside the array");
		std::vector<KdNode> bad = {KdNode{0u, (5u << 4) | 12u | 1u}};   // a branch whose children lie outside
		CHECK(kd_tree_shape(bad, 0) == 0u, "children outside the array");
	} catch (const Error& e) {
		fprintf(stderr, "error %d: %s\n", e.code, e.msg.c_str());
		return 2;
	}
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("kd_shapes_check: ok\n");
	return 0;
}
