// Pointer-free scene layout shared by the host builder and the HIP kernels.
//
// The reference keeps the scene as a shared_ptr graph (entity -> model -> surfaces -> mesh ->
// kd_tree_node, LIB/scene/entity.hpp, LIB/core/kd_tree.hpp:20-31). Here everything is a flat array:
// fixed-size records for models / surfaces / materials (read with scalar loads: the loop index is
// wave-uniform), 8-byte KD nodes, 4-byte leaf references and 48-byte triangle records (the three
// arrays the kernels stage through LDS), and 144-byte per-triangle hit records that stay in HBM/L2.
#pragma once
#include <cstdint>
#include <vector>
#include <string>

namespace ptx {

// ---- KD node: 2 dwords -------------------------------------------------------------------------
// word1[1:0] = kind: 0,1,2 = branch on that axis, 3 = leaf
// branch: word0 = split plane (float bits); word1 bit2 = has_left, bit3 = has_right,
//         word1[31:4] = index of the first existing child; the right child sits at +has_left.
//         (a missing child is the reference's nullptr child, mesh.cpp:227-241)
// leaf:   word0 = index of the first leaf reference; word1[31:2] = reference count
struct KdNode { uint32_t w0, w1; };
constexpr uint32_t KD_LEAF = 3u;
inline KdNode kd_make_branch(float split, uint32_t axis, bool has_l, bool has_r, uint32_t first_child) {
	uint32_t bits;
	__builtin_memcpy(&bits, &split, 4);
	return {bits, axis | (has_l ? 4u : 0u) | (has_r ? 8u : 0u) | (first_child << 4)};
}
inline KdNode kd_make_leaf(uint32_t first_ref, uint32_t count) { return {first_ref, KD_LEAF | (count << 2)}; }

// ---- triangle corner record (host side only: counts and inspection; the device reads HitRec) ----
// xyz = corner position (mesh-local space), w = bit pattern of the GLOBAL vertex id of that corner
struct TriRec { float ax, ay, az; uint32_t ia; float bx, by, bz; uint32_t ib; float cx, cy, cz; uint32_t ic; };

// ---- triangle intersection record: 3 x float4 (48 B), the form the traversal kernels stage through LDS:
// a.xyz, c3 | e1 = a-b | e2 = a-c, with c3 = e1.y*e2.z - e2.y*e1.z — the ray-independent sub-terms of the
// reference's Cramer solve (triangle.cpp:136-147: m.x = a-b, m.y = a-c, c3), computed once on the host with
// the same float operations (so the same bits) instead of once per ray-triangle test.
// Ordered for packed-fp32 math (v_pk_mul_f32 / v_pk_add_f32 take even-aligned register pairs): every pair the solve
// multiplies lane-wise sits in one 8-byte slot, so the three LDS / global reads deliver it ready to use.
struct TriIsect { float e2y, e1z, e2z, e1y; float e1x, e2x, ay, az; float ax, c3, p0, p1; };
// The record of the triangle (a, b, c) with global triangle id `gid` in its p0 word (what a hit reports): the one place records are
// made (scene_build.cpp), for finalize_scene and for ptx_leaf_intersect_batch.
TriIsect make_tri_isect(const float* a, const float* b, const float* c, uint32_t gid);

// ---- hit record: 9 x float4 (144 B) per triangle — everything renderer::intersect interpolates on a hit (renderer.cpp:688-715),
// gathered per triangle so that a hit costs ONE round of fetches: corners + u | normals + v | tangents. (Fetching the corner
// record first and the three vertices' attributes through its ids afterwards was two dependent rounds per shaded vertex.)
struct HitRec { float a[3], ua, b[3], ub, c[3], uc, na[3], va, nb[3], vb, nc[3], vc, ta[3], p0, tb[3], p1, tc[3], p2; };
static_assert(sizeof(HitRec) == 144, "HitRec layout");

// ---- per-model record (scene::model + its entity's global transform) ----
struct ModelRec {
	float inv_basis[9];   // columns x,y,z of inverse(basis)            — transform::inverse, transform.cpp:33-36
	float inv_origin[3];  // inverse(basis) * -origin
	float basis[9];       // columns of the global basis (local -> world; distance conversion model.cpp:62-63)
	float origin[3];
	float nmat[9];        // columns of transpose(inverse(basis))        — renderer.cpp:698
	float bmin[3], bmax[3];  // model AABB in local space                 — model.cpp:13-18
	int32_t first_surface, n_surfaces;
	float pbmin[3], pbmax[3];  // the box grown by the reach of the +-epsilon barycentric slack: every point the triangle tests of this
	                           // model can accept lies inside it (pruning of set-aside traversals, kernels.hip)
	float pad0;
	float box[6], pbox[6];     // the two boxes again as (min.x, max.x, min.y, max.y, min.z, max.z): the kernels' slab test works on (min, max)
	                           // pairs with packed fp32 instructions and takes each pair as one 64-bit scalar operand (interleave_boxes)
};
static_assert(sizeof(ModelRec) == 60 * 4, "ModelRec layout");

// ---- per-surface record (model::surface = mesh + material) ----
struct SurfaceRec {
	float bmin[3], bmax[3];  // mesh AABB (mesh.cpp:254-261)
	uint32_t kd_root;        // index of the root KD node in the full node array
	uint32_t tri_base;       // global id of the mesh's triangle 0
	uint32_t lds_root;       // 0xFFFFFFFF when the surface is not resident (tested first); else bits 28:0 (kLdsRootMask) = index of the root in the
	                         // LDS-resident node array, bit 31 (kLdsLeafOrderBit) = its resident records are leaf-ordered, bits 30 / 29
	                         // (kLdsLeafOnlyBit / kLdsCompleteBit) = the shape of its tree, set on leaf-ordered surfaces only (plan_residency)
	uint32_t model;          // the model this surface belongs to
	float pbmin[3], pbmax[3];  // mesh AABB grown by the reach of the barycentric slack (see ModelRec)
	float box[6], pbox[6];     // both boxes as (min, max) pairs per axis (see ModelRec)
};
static_assert(sizeof(SurfaceRec) == 28 * 4, "SurfaceRec layout");
constexpr uint32_t kLdsLeafOrderBit = 0x80000000u;
// The shape of a resident, leaf-ordered tree, read off its node words (kd_tree_shape). The surface record is scalar-loaded, so a kernel
// branches on these bits wave-uniformly, to a walk with the shape's constants folded in (device_core.hpp: mesh_traverse_m).
constexpr uint32_t kLdsLeafOnlyBit = 0x40000000u;   // the root is a leaf
constexpr uint32_t kLdsCompleteBit = 0x20000000u;   // every branch node has both children and no root-to-leaf path holds more than
                                                    // kShapeMaxBranchLevels branch nodes (never set together with kLdsLeafOnlyBit)
constexpr uint32_t kLdsRootMask = 0x1FFFFFFFu;
constexpr int kShapeMaxBranchLevels = 3;            // = kRegStack (device_core.hpp): one pending entry per branch level fits the register stack

// ---- auxiliary record per surface: flags that do not fit SurfaceRec, whose layout and lds_root word tests pin. A table of its own
// (FlatScene::surf_aux), passed to the fused kernels as a separate argument and scalar-loaded like the others.
struct UnitAux {
	uint32_t flags;    // kAuxChainBit
	uint32_t pad[3];
};
static_assert(sizeof(UnitAux) == 16, "UnitAux layout");
constexpr uint32_t kAuxChainBit = 1u;   // the resident, leaf-ordered tree is a chain (kd_chain_shape >= 0), walked by mesh_traverse_chain

template <class Rec> inline void interleave_boxes(Rec& r) {
	for (int k = 0; k < 3; k++) { r.box[2 * k] = r.bmin[k]; r.box[2 * k + 1] = r.bmax[k]; r.pbox[2 * k] = r.pbmin[k]; r.pbox[2 * k + 1] = r.pbmax[k]; }
}

// ---- what a path vertex computes from the material's roughness and ior alone (core/pbr.cpp:13-25, 79-91, 104-114, 125-140, 172-184).
// One definition for both sides: the kernels evaluate these per vertex where a texture can scale the roughness, and the scene builder
// evaluates them once per surface into the shade record, which the untextured kernels read instead (-DPTX_NO_SHADE_CONSTS: they
// evaluate them too). IEEE binary32, one rounding per operation on the host as on the device (-ffp-contract=off), so the record
// holds the bits the vertex would compute.
#ifdef __HIP__
#define PTX_HD __attribute__((host)) __attribute__((device))
#else
#define PTX_HD
#endif
struct RoughConsts { float r4, r4m1, smith_k; };   // roughness^4, roughness^4 - 1, (roughness + 1)^2 / 8
PTX_HD inline float pmax_hd(float a, float b) { return b > a ? b : a; }   // math::max (NaN-asymmetric), math.inl:169: the device's pmax
PTX_HD inline float clamp_roughness(float roughness) { return pmax_hd(roughness, 0.05F); }   // renderer.cpp:486
PTX_HD inline RoughConsts rough_consts(float roughness) {   // of the clamped roughness
	RoughConsts c;
	c.r4 = roughness * roughness;
	c.r4 *= c.r4;
	c.r4m1 = c.r4 - 1;
	const float r = roughness + 1;
	c.smith_k = (r * r) / 8;
	return c;
}
PTX_HD inline float fresnel_f0sq(float ior) {
	float f0 = (ior - 1) / (ior + 1);
	f0 *= f0;
	return f0;
}

// ---- what a model's transform determines: the five groups of floats of ModelRec / SpaceRec / ShadeRec. One definition for both sides,
// as rough_consts is: apply_model_xforms calls it per model, and under motion (include/ptx.h: MOTION) a lane calls it on the transform
// of its own time. IEEE binary32, one rounding per operation, in the reference's order (transform::inverse, transform.cpp:33-36; mat3
// inverse, mat3.inl:245-263; rows dotted with v, mat3.inl:219-224), so both sides hold the same bits. Written without loops or indexed
// temporaries: on the device every value stays in a register.
struct XformRecs {
	float basis[9], origin[3];       // the transform itself: columns of the basis, origin
	float inv_basis[9], inv_origin[3];
	float nmat[9];                   // transpose(inverse(basis)), columns
};
PTX_HD inline void mat_inverse_hd(const float* m, float* out) {
	const float xx = m[0], xy = m[1], xz = m[2], yx = m[3], yy = m[4], yz = m[5], zx = m[6], zy = m[7], zz = m[8];
	const float det1 = +(yy * zz - zy * yz);
	const float det2 = -(xy * zz - zy * xz);
	const float det3 = +(xy * yz - yy * xz);
	const float det = xx * det1 + yx * det2 + zx * det3;
	const float s = 1 / det;
	out[0] = det1 * s; out[1] = det2 * s; out[2] = det3 * s;
	out[3] = (-(yx * zz - zx * yz)) * s; out[4] = (+(xx * zz - zx * xz)) * s; out[5] = (-(xx * yz - yx * xz)) * s;
	out[6] = (+(yx * zy - zx * yy)) * s; out[7] = (-(xx * zy - zx * xy)) * s; out[8] = (+(xx * yy - yx * xy)) * s;
}
// x: [12] origin, basis columns (PTX_ARR_MODEL_XFORM's layout)
PTX_HD inline void derive_xform(const float* x, XformRecs& r) {
	r.origin[0] = x[0]; r.origin[1] = x[1]; r.origin[2] = x[2];
	r.basis[0] = x[3]; r.basis[1] = x[4]; r.basis[2] = x[5]; r.basis[3] = x[6]; r.basis[4] = x[7]; r.basis[5] = x[8];
	r.basis[6] = x[9]; r.basis[7] = x[10]; r.basis[8] = x[11];
	mat_inverse_hd(r.basis, r.inv_basis);
	const float n0 = -x[0], n1 = -x[1], n2 = -x[2];
	const float* m = r.inv_basis;
	r.inv_origin[0] = m[0] * n0 + m[3] * n1 + m[6] * n2;
	r.inv_origin[1] = m[1] * n0 + m[4] * n1 + m[7] * n2;
	r.inv_origin[2] = m[2] * n0 + m[5] * n1 + m[8] * n2;
	// column k of the transpose is row k of the inverse
	r.nmat[0] = m[0]; r.nmat[1] = m[3]; r.nmat[2] = m[6];
	r.nmat[3] = m[1]; r.nmat[4] = m[4]; r.nmat[5] = m[7];
	r.nmat[6] = m[2]; r.nmat[7] = m[5]; r.nmat[8] = m[8];
}
// The state of a moving transform (or camera) at time u: x(u)[k] = a[k] + (b[k] - a[k]) * u, a the begin and b the current value
PTX_HD inline float motion_mix(float a, float b, float u) { return a + (b - a) * u; }
PTX_HD inline void motion_xform(const float* a, const float* b, float u, float* x) {
	x[0] = motion_mix(a[0], b[0], u); x[1] = motion_mix(a[1], b[1], u); x[2] = motion_mix(a[2], b[2], u); x[3] = motion_mix(a[3], b[3], u);
	x[4] = motion_mix(a[4], b[4], u); x[5] = motion_mix(a[5], b[5], u); x[6] = motion_mix(a[6], b[6], u); x[7] = motion_mix(a[7], b[7], u);
	x[8] = motion_mix(a[8], b[8], u); x[9] = motion_mix(a[9], b[9], u); x[10] = motion_mix(a[10], b[10], u); x[11] = motion_mix(a[11], b[11], u);
}

// ---- material factors (core/material.hpp:11-17) and texture slots ----
struct MaterialRec {
	float albedo[3]; float opacity;
	float emissive[3]; float roughness;   // emissive factor; the shader multiplies the looked-up value by 10 (renderer.cpp:462)
	float metallic; float ior; uint32_t shadow_catcher; uint32_t tex_mask;
	int32_t tex[7];   // texture id per slot: normal, albedo, opacity, occlusion, roughness, metallic, emissive; -1 = none
	float f0sq;       // fresnel_f0sq(ior)
};
static_assert(sizeof(MaterialRec) == 80, "MaterialRec layout");

// ---- texture: 8-bit texels exactly as the reference keeps them (image::image::data, image.cpp:124-141); the sRGB
// decode pow(v/255, 2.2) of colour channels is a 256-entry table computed on the host with the same libm call.
// A Radiance .hdr image keeps its floats (image::read returns them unscaled): c_srgb bit 16, offset counts floats in `texels_f`.
struct TexRec { uint32_t w, h, c_srgb /* channels | srgb << 8 | float texels << 16 */, offset /* first byte in the texel array (first float for float texels) */; };
constexpr uint32_t kTexSrgb = 1u << 8, kTexFloat = 1u << 16;

// ---- everything the SHADING phase needs about the surface that was hit, gathered per surface so that a
// divergent lookup is 9 aligned 16-byte reads from one place (LDS when it fits): the owning model's
// local->world transform and normal matrix, and the material. 176 B.
struct ShadeRec {
	float basis[9];   // model global basis, columns
	float origin[3];
	float nmat[9];    // transpose(inverse(basis)), columns
	RoughConsts rc;   // rough_consts(clamp_roughness(mat.roughness)): the factor's, valid where no texture scales it
	MaterialRec mat;
};
// the constants of a surface's material, as the untextured vertex would compute them
inline void fill_shade_consts(ShadeRec& r) {
	r.rc = rough_consts(clamp_roughness(r.mat.roughness));
	r.mat.f0sq = fresnel_f0sq(r.mat.ior);
}
static_assert(sizeof(ShadeRec) == 176 && sizeof(ShadeRec) % 16 == 0, "ShadeRec layout: staged into LDS in 16-byte units");

// ---- ray space: a distinct world->local transform. Models whose entity transforms are bitwise equal
// share one, so the local ray (origin, normalised direction, reciprocal direction) is computed once per
// space instead of once per model (model.cpp:22-29 recomputes it per model; same operations, same bits).
struct SpaceRec {
	float inv_basis[9];
	float inv_origin[3];
};

// The lens fields (ptx_scene_set_camera, include/ptx.h: THE LENS) are all zero on a scene never given a lens: lens_radius == 0 is the pinhole.
struct CameraRec { float origin[3]; float basis[9]; float fov; float tan_half_fov; float lens_radius, focus_distance; uint32_t blades; float blade_rotation; };
constexpr uint32_t kLensMaxBlades = 32;   // the aperture table holds blades + 1 corners, the last a copy of the first
struct SunRec { float basis[9]; float energy[3]; float angular_radius; uint32_t present; };

// ---- host-side container ----
struct FlatScene {
	// description as loaded (kept for inspection / tests)
	std::vector<std::string> model_names;
	std::vector<float> model_xform;      // [n][12]
	std::vector<int32_t> model_surf;     // [n][2]
	std::vector<int32_t> surf_range;     // [ns][8]: v0,nv,t0,nt,kd_root,n_nodes,ref0,n_refs
	std::vector<float> vertices;         // [nv][11]
	std::vector<uint32_t> triangles;     // [nt][3] mesh-local ids
	std::vector<float> materials_raw;    // [ns][11]
	std::vector<uint8_t> material_tex;   // [ns][7] texture present per slot
	std::vector<int32_t> surf_tex;       // [ns][7] texture id per slot or -1
	std::vector<TexRec> textures;
	std::vector<uint8_t> texels;
	std::vector<float> texels_f;         // texels of .hdr images
	std::vector<std::string> texture_paths;
	// derived, device-ready
	std::vector<ModelRec> models;
	std::vector<SurfaceRec> surfaces;
	std::vector<MaterialRec> materials;
	std::vector<ShadeRec> shade;         // per surface
	std::vector<SpaceRec> spaces;        // distinct world->local transforms
	std::vector<uint32_t> model_space;   // per model
	std::vector<UnitAux> surf_aux;       // per surface: chain flag (plan_residency)
	std::vector<KdNode> kd_nodes;
	std::vector<uint32_t> kd_refs;       // global triangle ids
	std::vector<TriRec> tris;            // corners + vertex ids (host side: counts, inspection)
	std::vector<TriIsect> tri_isect;     // intersection form (traversal)
	std::vector<HitRec> hitrec;          // per triangle: what a hit interpolates (shading)
	std::vector<HitRec> hot_hitrec;      // the hit records kept in LDS beside the resident geometry (largest triangles first; upload_scene)
	CameraRec camera{};
	SunRec sun{};
	// ptx_scene_set_motion (include/ptx.h: MOTION): the state at u = 0; the scene's own camera and transforms are the state at u = 1.
	// `set`: a call is in force (the inspection arrays are non-empty); active(): some model or the camera moves.
	struct Motion {
		bool set = false, camera_moved = false;
		std::vector<float> begin_xform;    // [n][12]; a static model's entry is a bitwise copy of its current transform
		std::vector<uint32_t> moved;       // [n] 1: the begin transform differs bitwise from the current one
		float begin_camera[12] = {};       // origin, basis; the current camera's when it does not move
		float shutter_open = 0, shutter_close = 1;
		bool any_model() const { for (uint32_t m : moved) if (m) return true; return false; }
		bool active() const { return set && (camera_moved || any_model()); }
	} motion;
	uint32_t kd_max_depth = 0;
	bool any_texture = false;
	bool any_alpha = false;              // some material can take the opacity / shadow-catcher pass-through branch
	int32_t env_tex = -1;                // renderer::environment: index into `textures`, -1 = none

	// LDS residency plan (plan_residency): the traversal arrays of the surfaces that fit one CU's LDS, indices local to them
	std::vector<KdNode> res_nodes;
	std::vector<uint32_t> res_refs;      // indices into res_tris (ref-indexed surfaces only)
	std::vector<TriIsect> res_tris;      // p0 = global triangle id; per triangle (ref-indexed surface) or per leaf reference (leaf-ordered one)
	uint32_t n_resident = 0;             // surfaces with SurfaceRec::lds_root valid
	size_t res_bytes = 0;                // LDS bytes the resident arrays + shade records take

	size_t geometry_bytes() const { return kd_nodes.size() * 8 + kd_refs.size() * 4 + tris.size() * 48; }
};

// Chooses which surfaces are staged into LDS (smallest first, while they fit `lds_budget` together with the shade records)
// and builds their compact arrays; sets SurfaceRec::lds_root. With `lds_leaf_order`, the resident surfaces whose records cost little
// more per leaf reference than per triangle get the leaf-ordered layout (bit 31 of lds_root): their leaves index res_tris directly, one
// record per reference, and they add nothing to res_refs. Ref-indexed surfaces keep one record per triangle behind res_refs. The two
// kinds share the three arrays, so the compact arrays differ from the full ones even when every surface is resident.
constexpr size_t kLdsLeafOrderCap = 4096;   // bytes the leaf-ordered layouts may cost together: 28 hot hit records (144 B) at the most
// With `kd_shapes`, the leaf-ordered surfaces also get the shape bits of their trees (kLdsLeafOnlyBit / kLdsCompleteBit), and kAuxChainBit
// in surf_aux (sized and zeroed here) where the tree is a chain.
void plan_residency(FlatScene& s, size_t lds_budget, bool lds_leaf_order = true, bool kd_shapes = true);
// kLdsLeafOnlyBit, kLdsCompleteBit or 0 for the tree at `root` of `nodes` (children at w1 >> 4, adjacent; w1 & 4 / & 8: left / right present)
uint32_t kd_tree_shape(const std::vector<KdNode>& nodes, uint32_t root);
// A chain: every node from `root` down is a branch with exactly one child, ending in a leaf. Returns its number of branch levels (0: the root
// is a leaf), or -1 when the tree is no chain or an index leaves the array.
int kd_chain_shape(const std::vector<KdNode>& nodes, uint32_t root);

// Builds everything derived (AABBs, KD-trees, records) from the "as loaded" arrays + camera/sun floats.
// camera13: origin(3) basis(9) fov ; sun13: basis(9) energy(3) angular_radius or nullptr.
void finalize_scene(FlatScene& s, const float* camera13, const float* sun13);
// The transform-dependent tail of finalize_scene, from s.model_xform: model records (inverse and normal matrices, boxes), the distinct ray
// spaces, and the shade records. Builds no tree; ptx_scene_set_model_xforms reruns it on a finished scene.
void apply_model_xforms(FlatScene& s);
// The distinct ray spaces (s.spaces, s.model_space) from the model records. Models share one when their inverse transforms are bitwise
// equal and neither moves (s.motion); two moving models only when their begin and their current transforms are bitwise equal as well; a
// moving model never shares one with a static model. Without motion: the spaces apply_model_xforms has always made.
void assign_ray_spaces(FlatScene& s);
// The aperture table of a camera with a lens (include/ptx.h: THE APERTURE TABLE): blades + 1 corners (x, y), float64 arithmetic, stored as
// float32, the last entry a bitwise copy of the first. Empty when lens_radius == 0.
std::vector<float> lens_table(const CameraRec& cam);

// glTF loader (throws ptx::Error)
struct Error {
	int code;
	std::string msg;
};
void read_png(const std::string& path, uint32_t& W, uint32_t& H, uint32_t& C, std::vector<uint8_t>& out);
void read_jpeg(const std::string& path, uint32_t& W, uint32_t& H, uint32_t& C, std::vector<uint8_t>& out);    // jpeg_read.cpp
bool is_hdr_file(const std::string& path);                                                                      // hdr_read.cpp
void read_hdr(const std::string& path, uint32_t& W, uint32_t& H, uint32_t& C, std::vector<float>& out);
void read_image(const std::string& path, uint32_t& W, uint32_t& H, uint32_t& C, std::vector<uint8_t>& out);   // PNG or JPEG, by content
// image::image::load: appends the image's texels to the scene's arrays (8-bit ones to `texels`, .hdr floats to `texels_f`) and returns its record
TexRec load_texture(FlatScene& s, const std::string& path, bool srgb);
// work: the host's `scene_info.work` primitive filter (src/models/work_info.hpp:11-15, src/scene/load_gltf.cpp:95-99):
// when `filter` is set, only the listed primitive indices of each named mesh are loaded (a mesh that is not listed
// loads nothing but keeps its model); when clear, every primitive is loaded (core::renderer::load_gltf).
struct WorkFilter {
	bool filter = false;
	std::vector<std::pair<std::string, std::vector<int32_t>>> work;
};
void load_gltf(const std::string& path, uint32_t camera_index, uint32_t sun_light_index, const WorkFilter& work, FlatScene& out);
// the file's point and spot lights, 16 floats each (include/ptx.h: ptx_gltf_read_punctual_lights); reads the .gltf only, no buffer or image
void read_gltf_punctual_lights(const std::string& path, std::vector<float>& out);

// The Lambda event of the reference's worker (models::worker_info, src/models/work_info.hpp:17-32; sample:
// path-tracer-core/events/event.json)
struct WorkerEvent {
	WorkFilter work;
	std::string scene_bucket, scene_root, worker_id;
	int32_t num_workers = 1, samples = 0, bounces = 0;
	float X = 0, Y = 0;
};
void parse_worker_event(const std::string& json_path, WorkerEvent& out);

}  // namespace ptx
