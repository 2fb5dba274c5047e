// Stand-alone host check of the per-material shade constants (flat_scene.hpp: fill_shade_consts, called by scene_build.cpp): the records
// of the Cornell box as the scene builder leaves them, and a grid of corner materials (zeros, the roughness clamp, a zero denominator,
// denormals, infinities, NaN), against the expressions written out once more here. Meant to be built with -fsanitize=address,undefined
// and run on the CPU (`make -C distributed-path-tracer_amd/csrc consts_check`). Usage: shade_consts_check <cornell.gltf>. Exit status 0 =
// every check held.
#include "../distributed-path-tracer_amd/csrc/flat_scene.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace ptx;

static int g_fail = 0;

static bool same(float a, float b) { return !memcmp(&a, &b, 4) || (std::isnan(a) && std::isnan(b)); }

// renderer.cpp:486, pbr.cpp:13-25, 79-91, 104-114, 125-140 — one statement per operation
static void expect(const ShadeRec& r, const char* what, size_t k) {
	const float rough = 0.05F > r.mat.roughness ? 0.05F : r.mat.roughness;
	const float r2 = rough * rough;
	const float r4 = r2 * r2;
	const float r4m1 = r4 - 1.0F;
	const float rp = rough + 1.0F;
	const float rp2 = rp * rp;
	const float k8 = rp2 / 8.0F;
	const float num = r.mat.ior - 1.0F, den = r.mat.ior + 1.0F;
	const float f0 = num / den;
	const float f0sq = f0 * f0;
	if (!same(r.rc.r4, r4) || !same(r.rc.r4m1, r4m1) || !same(r.rc.smith_k, k8) || !same(r.mat.f0sq, f0sq)) {
		g_fail++;
		fprintf(stderr, "FAIL %s %zu: roughness %a ior %a: record (%a %a %a %a), expected (%a %a %a %a)\n", what, k, r.mat.roughness, r.mat.ior,
		        r.rc.r4, r.rc.r4m1, r.rc.smith_k, r.mat.f0sq, r4, r4m1, k8, f0sq);
	}
}

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s <cornell.gltf>\n", argv[0]); return 2; }
	try {
		FlatScene cornell;
		load_gltf(argv[1], 0u, 0u, WorkFilter{}, cornell);
		for (size_t k = 0; k < cornell.shade.size(); k++) {
			expect(cornell.shade[k], "cornell surface", k);
			if (!same(cornell.materials[k].f0sq, cornell.shade[k].mat.f0sq)) { g_fail++; fprintf(stderr, "FAIL cornell surface %zu: material and shade record disagree\n", k); }
		}
		printf("cornell: %zu shade records\n", cornell.shade.size());
	} catch (const Error& e) {
		fprintf(stderr, "error %d: %s\n", e.code, e.msg.c_str());
		return 2;
	}
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), dn = std::numeric_limits<float>::denorm_min();
	const float vals[] = {0.0F, -0.0F, 0.0499F, 0.05F, 0.5F, 1.0F, 1.45F, -1.0F, dn, -dn, 1e-39F, std::numeric_limits<float>::max(), inf, -inf, nan};
	std::vector<ShadeRec> recs;
	for (float rough : vals)
		for (float ior : vals) {
			ShadeRec r{};
			r.mat.roughness = rough; r.mat.ior = ior;
			recs.push_back(r);
		}
	for (ShadeRec& r : recs) fill_shade_consts(r);
	for (size_t k = 0; k < recs.size(); k++) expect(recs[k], "grid material", k);
	printf("grid: %zu materials\n", recs.size());
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("shade_consts_check: ok\n");
	return 0;
}
