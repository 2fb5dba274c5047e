// Stand-alone host check of the motion-blur derivation (flat_scene.hpp: motion_xform, derive_xform; scene_build.cpp: apply_model_xforms,
// assign_ray_spaces). The kernels derive a moving model's records per lane with derive_xform on x(u) = a + (b - a) * u; this program checks
// that those are, bit for bit, what apply_model_xforms leaves in ModelRec and ShadeRec for a scene given x(u), against the inverse, the
// matrix-vector product and the transpose written out once more here, a singular matrix included; and that the ray-space rule keeps two
// models apart that are equal at the end of the motion only. Meant to be built with -fsanitize=address,undefined and run on the CPU
// (`make -C distributed-path-tracer_amd/csrc motion_check`). Usage: motion_check <cornell.gltf>. Exit status 0 = every check held.
#include "../distributed-path-tracer_amd/csrc/flat_scene.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ptx;

static int g_fail = 0;

static bool same(const float* a, const float* b, int n) {
	for (int k = 0; k < n; k++)
		if (memcmp(a + k, b + k, 4) && !(std::isnan(a[k]) && std::isnan(b[k]))) return false;
	return true;
}
static void check(bool ok, const char* what, size_t k, float u) {
	if (ok) return;
	g_fail++;
	fprintf(stderr, "FAIL %s (model %zu, u = %a)\n", what, k, u);
}

// transform::inverse (transform.cpp:33-36) over the mat3 inverse (mat3.inl:245-263) and rows dotted with v (mat3.inl:219-224), with loops
// and temporaries as the scene builder had them before the derivation became shared
static void expect_records(const float* x, float* inv, float* inv_origin, float* nmat) {
	const float* m = x + 3;
	const float xx = m[0], xy = m[1], xz = m[2], yx = m[3], yy = m[4], yz = m[5], zx = m[6], zy = m[7], zz = m[8];
	float det1 = +(yy * zz - zy * yz);
	float det2 = -(xy * zz - zy * xz);
	float det3 = +(xy * yz - yy * xz);
	float det = xx * det1 + yx * det2 + zx * det3;
	float s = 1 / det;
	float r[9] = {det1, det2, det3, -(yx * zz - zx * yz), +(xx * zz - zx * xz), -(xx * yz - yx * xz), +(yx * zy - zx * yy), -(xx * zy - zx * xy), +(xx * yy - yx * xy)};
	for (int k = 0; k < 9; k++) inv[k] = r[k] * s;
	const float neg[3] = {-x[0], -x[1], -x[2]};
	for (int row = 0; row < 3; row++) inv_origin[row] = inv[row] * neg[0] + inv[3 + row] * neg[1] + inv[6 + row] * neg[2];
	for (int c = 0; c < 3; c++)
		for (int row = 0; row < 3; row++) nmat[3 * c + row] = inv[3 * row + c];
}

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s <cornell.gltf>\n", argv[0]); return 2; }
	try {
		FlatScene s;
		load_gltf(argv[1], 0u, 0u, WorkFilter{}, s);
		const size_t n = s.model_xform.size() / 12;
		if (n < 4) { fprintf(stderr, "the scene has fewer than four models\n"); return 2; }
		const std::vector<float> b = s.model_xform;
		std::vector<float> a = b;
		for (size_t k = 0; k < n; k++) {   // begin keys: every model displaced, turned a little and scaled; model 1 ends singular at u = 0.5
			float* x = &a[12 * k];
			x[0] += 0.25f * (float)(k + 1); x[1] -= 0.1f; x[2] += 0.05f * (float)k;
			const float c = std::cos(0.2f * (float)(k + 1)), sn = std::sin(0.2f * (float)(k + 1));
			for (int col = 0; col < 3; col++) {
				const float vx = x[3 + 3 * col], vz = x[5 + 3 * col];
				x[3 + 3 * col] = (c * vx + sn * vz) * 0.8f;
				x[5 + 3 * col] = (c * vz - sn * vx) * 0.8f;
			}
		}
		for (int k = 3; k < 12; k++) a[12 + k] = -b[12 + k];   // a half-turn and a reflection: the blend at u = 0.5 is the zero matrix
		const float us[] = {0.0f, 0.3f, 0.5f, 0.75f, 1.0f, 0.123456f};
		for (float u : us) {
			std::vector<float> xu(12 * n);
			for (size_t k = 0; k < n; k++) {
				motion_xform(&a[12 * k], &b[12 * k], u, &xu[12 * k]);
				for (int j = 0; j < 12; j++) {   // the formula, once more
					const float e = a[12 * k + j] + (b[12 * k + j] - a[12 * k + j]) * u;
					check(same(&e, &xu[12 * k + j], 1), "motion_xform is not a + (b - a) * u", k, u);
				}
			}
			s.model_xform = xu;
			apply_model_xforms(s);
			for (size_t k = 0; k < n; k++) {
				XformRecs r;
				derive_xform(&xu[12 * k], r);   // what a lane computes
				float inv[9], io[3], nm[9];
				expect_records(&xu[12 * k], inv, io, nm);
				const ModelRec& M = s.models[k];
				check(same(r.inv_basis, inv, 9) && same(r.inv_origin, io, 3) && same(r.nmat, nm, 9), "derive_xform differs from the written-out derivation", k, u);
				check(same(M.basis, r.basis, 9) && same(M.origin, r.origin, 3), "ModelRec basis / origin", k, u);
				check(same(M.inv_basis, r.inv_basis, 9) && same(M.inv_origin, r.inv_origin, 3), "ModelRec inverse", k, u);
				check(same(M.nmat, r.nmat, 9), "ModelRec nmat", k, u);
				for (int32_t q = 0; q < M.n_surfaces; q++) {
					const ShadeRec& R = s.shade[M.first_surface + q];
					check(same(R.basis, r.basis, 9) && same(R.origin, r.origin, 3) && same(R.nmat, r.nmat, 9), "ShadeRec", k, u);
				}
				const SpaceRec& SP = s.spaces[s.model_space[k]];
				check(same(SP.inv_basis, r.inv_basis, 9) && same(SP.inv_origin, r.inv_origin, 3), "SpaceRec", k, u);
			}
		}
		printf("records: %zu models at %zu times\n", n, sizeof us / sizeof us[0]);

		// the ray spaces: models 0 and 1 equal at the end only, models 2 and 3 equal in both keys
		std::vector<float> cur = b;
		memcpy(&cur[12], &cur[0], 48);
		memcpy(&cur[36], &cur[24], 48);
		s.model_xform = cur;
		s.motion = FlatScene::Motion{};
		apply_model_xforms(s);
		check(s.model_space[0] == s.model_space[1] && s.model_space[2] == s.model_space[3], "static models with equal transforms share a ray space", 0, 1.0f);
		const std::vector<uint32_t> static_spaces = s.model_space;
		FlatScene::Motion mo;
		mo.set = true;
		mo.begin_xform = cur;
		mo.moved.assign(n, 0u);
		mo.begin_xform[0] += 1.0f; mo.moved[0] = 1u;                    // 0 and 1 come from different places
		mo.begin_xform[12] -= 1.0f; mo.moved[1] = 1u;
		mo.begin_xform[24] += 0.5f; mo.moved[2] = 1u;                   // 2 and 3 travel together
		mo.begin_xform[36] += 0.5f; mo.moved[3] = 1u;
		s.motion = mo;
		assign_ray_spaces(s);
		check(s.model_space[0] != s.model_space[1], "models equal at the end only must not share a ray space", 0, 1.0f);
		check(s.model_space[2] == s.model_space[3], "models equal in both keys share a ray space", 2, 1.0f);
		for (size_t k = 0; k < n; k++) check(s.model_space[k] < s.spaces.size(), "model_space out of range", k, 1.0f);
		s.motion.moved[1] = 0u;                                          // a moving and a static model never share one
		memcpy(&s.motion.begin_xform[12], &cur[12], 48);
		assign_ray_spaces(s);
		check(s.model_space[0] != s.model_space[1], "a moving and a static model must not share a ray space", 0, 1.0f);
		s.motion = FlatScene::Motion{};
		assign_ray_spaces(s);
		check(s.model_space == static_spaces, "cleared motion gives the static spaces back", 0, 1.0f);
		printf("ray spaces: ok\n");
	} catch (const Error& e) {
		fprintf(stderr, "error %d: %s\n", e.code, e.msg.c_str());
		return 2;
	}
	if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("motion_check: ok\n");
	return 0;
}
