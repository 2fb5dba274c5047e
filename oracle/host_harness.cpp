// TEST INFRASTRUCTURE — drives the UNMODIFIED HOST worker of the reference (src/processors/worker/*.cpp, src/scene/*.cpp, compiled
// from where they lie by oracle/Makefile, target `ref-host`, against the stand-in headers of oracle/host_stubs/) on ONE thread, to
// produce the fixtures that pin the oracle's worker estimator (ora_trace_worker_mt) and the loader's primitive filter.
//
// Nothing in here is reference code: it calls processors::worker's own stage functions (this file alone is compiled with
// -fno-access-control) and supplies what the worker expects from its surroundings:
//   cloud::s3_download_object   a path output is a no-op (the buffer lies beside the glTF), a byte output reads <glTF dir>/<key>
//   cloud::s3_upload_object     no-op
//   nanosleep                   no-op: the stage loops sleep 1 ms whenever a queue is empty
//   std::random_device          ORACLE_SEED + 7919 * k for the k-th stream that is seeded
// The queues are the single-threaded FIFO of host_stubs/concurrentqueue: an empty try_dequeue sets m_should_terminate, so a stage
// function returns once its queue is dry. A sample goes through ALONE: one cloud_ray is enqueued, the five stage functions are called
// in pipeline order until all five work queues are empty, then the one finished cloud_ray is taken from m_accumulate_queue. Each of
// the three core::rand() streams (one `static` copy per translation unit: worker.cpp = jitter, intersection_worker.cpp = sun cone,
// shading_worker.cpp = shading) is therefore drawn path after path.
//
// Sub-commands (each writes .npy files into <out>):
//   worker-frame <gltf> <out> <X> <Y> <spp> <bounces>   generate_rays() as it is; per sample in its order (x outer, y, sample):
//                                                       wf_uuid [n] u8, wf_rays [n][6], wf_out [n][4] (colour, alpha), wf_meta
//   worker-trace <gltf> <out> <seed> <n> <bounces>      n harness-made rays (ref_harness `trace`'s generator), each in a cloud_ray
//                                                       filled as generate_rays fills it: wt_rays, wt_out, wt_meta
//   worker-scene <gltf> <out> [mesh=i,j,...]...         the loaded distributed_scene in ref_harness `scene`'s layout, and intersect()
//                                                       / intersect_min_result() records of a stored ray batch (ws_rays, ws_out, ws_min)
// meta = [ORACLE_SEED, k_jitter, k_sun, k_shading (0xFFFFFFFF: never seeded), X, Y, spp, bounces]

#include "processors/worker/worker.hpp"
#include <path_tracer/core/utils.hpp>

#include <cstring>
#include <ctime>
#include <iostream>

using namespace math;

// ---- deterministic seeding of every thread_local mt19937 (core/utils.hpp:9) ----
static unsigned g_seed_calls = 0;
static unsigned seed_base() {
	const char* s = getenv("ORACLE_SEED");
	return s ? (unsigned)strtoul(s, nullptr, 10) : 12345u;
}
unsigned int std::random_device::_M_getval() { return seed_base() + 7919u * g_seed_calls++; }

extern "C" int nanosleep(const struct timespec*, struct timespec*) { return 0; }

static std::filesystem::path g_gltf_dir;
namespace cloud {
void s3_download_object(const std::string&, const std::string& key, std::variant<std::filesystem::path, std::vector<uint8_t>>& output) {
	if (output.index() == 0) return;
	std::ifstream f(g_gltf_dir / key, std::ios::binary);
	if (!f) throw std::runtime_error("host_harness: cannot read " + (g_gltf_dir / key).string());
	std::get<1>(output).assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
void s3_upload_object(const std::string&, const std::string&, std::variant<std::filesystem::path, std::vector<uint8_t>>&) {}
}  // namespace cloud

// ---- tiny .npy writer ----
static void save_npy(const std::string& path, const char* descr, const std::vector<size_t>& shape, const void* data, size_t bytes) {
	std::string shp = "(";
	for (size_t i = 0; i < shape.size(); i++) shp += std::to_string(shape[i]) + ",";
	shp += ")";
	std::string hdr = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shp + ", }";
	size_t total = 10 + hdr.size() + 1;
	size_t pad = (64 - total % 64) % 64;
	hdr += std::string(pad, ' ') + "\n";
	std::ofstream f(path, std::ios::binary);
	const char magic[] = "\x93NUMPY\x01\x00";
	f.write(magic, 8);
	uint16_t hl = (uint16_t)hdr.size();
	f.write((const char*)&hl, 2);
	f.write(hdr.data(), hdr.size());
	f.write((const char*)data, bytes);
}
template <typename T> static const char* descr_of();
template <> const char* descr_of<float>() { return "<f4"; }
template <> const char* descr_of<uint32_t>() { return "<u4"; }
template <> const char* descr_of<int32_t>() { return "<i4"; }
template <> const char* descr_of<uint64_t>() { return "<u8"; }
template <> const char* descr_of<uint8_t>() { return "|u1"; }
template <typename T>
static void save(const std::string& dir, const std::string& name, const std::vector<T>& v, std::vector<size_t> shape = {}) {
	if (shape.empty()) shape = {v.size()};
	save_npy(dir + "/" + name + ".npy", descr_of<T>(), shape, v.data(), v.size() * sizeof(T));
}

// ---- input generator (harness-owned PCG32; inputs are stored with the outputs) ----
struct pcg32 {
	uint64_t state, inc;
	explicit pcg32(uint64_t seed) : state(0), inc((seed << 1) | 1) { next(); state += 0x853c49e6748fea9bULL; next(); }
	uint32_t next() {
		uint64_t old = state;
		state = old * 6364136223846793005ULL + inc;
		uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
		uint32_t rot = (uint32_t)(old >> 59u);
		return (xs >> rot) | (xs << ((32 - rot) & 31));
	}
	float uni() { return (next() >> 8) * (1.0f / 16777216.0f); }
	float range(float a, float b) { return a + (b - a) * uni(); }
	fvec3 vec(float a, float b) { float x = range(a, b), y = range(a, b), z = range(a, b); return fvec3(x, y, z); }
};
static void push3(std::vector<float>& o, const fvec3& v) { o.push_back(v.x); o.push_back(v.y); o.push_back(v.z); }

// ---- the worker under the harness ----
static processors::worker* g_worker = nullptr;
static void queue_ran_dry() { if (g_worker) g_worker->m_should_terminate = true; }

struct model_ref { scene::entity* ent; std::shared_ptr<scene::model> model; };
// the order distributed_scene::intersect visits models in (src/scene/intersect.cpp:83-99)
static std::vector<model_ref> visit_order(const cloud::distributed_scene& sc) {
	std::vector<model_ref> out;
	std::stack<scene::entity*> stack;
	for (const auto& [_, e] : sc.m_entities) stack.push(e.get());
	while (!stack.empty()) {
		scene::entity* e = stack.top();
		stack.pop();
		for (const auto& c : e->get_children()) stack.push(c.get());
		if (auto m = e->get_component<scene::model>()) out.push_back({e, m});
	}
	return out;
}

// "mesh=0,2" arguments -> scene_work; none: every primitive of every mesh of the file
static std::map<mesh_name, primitives> parse_work(const char* gltf, int argc, char** argv, int first) {
	std::map<mesh_name, primitives> work;
	if (first < argc) {
		for (int i = first; i < argc; i++) {
			std::string a = argv[i];
			size_t eq = a.rfind('=');
			if (eq == std::string::npos) throw std::runtime_error("work argument is not mesh=i,j,...: " + a);
			primitives& p = work[a.substr(0, eq)];
			std::stringstream ss(a.substr(eq + 1));
			std::string tok;
			while (std::getline(ss, tok, ',')) if (!tok.empty()) p.push_back(atoi(tok.c_str()));
		}
		return work;
	}
	cgltf_options options = {};
	cgltf_data* data = nullptr;
	if (cgltf_parse_file(&options, gltf, &data) != cgltf_result_success) throw std::runtime_error("cannot parse the glTF");
	for (size_t m = 0; m < data->meshes_count; m++) {
		primitives& p = work[data->meshes[m].name ? data->meshes[m].name : ""];
		for (size_t k = 0; k < data->meshes[m].primitives_count; k++) p.push_back((int)k);
	}
	cgltf_free(data);
	return work;
}

struct rig {
	std::unique_ptr<processors::worker> w;
	uint32_t k_jitter = 0xFFFFFFFFu, k_sun = 0xFFFFFFFFu, k_shading = 0xFFFFFFFFu;

	rig(const char* gltf, const std::map<mesh_name, primitives>& work, uint32_t X, uint32_t Y, uint32_t spp, uint32_t bounces) {
		g_gltf_dir = std::filesystem::path(gltf).parent_path();
		models::worker_info info{};
		info.num_workers = 1;
		info.scene_info.work = work;
		w = std::make_unique<processors::worker>(info);
		std::cout.setstate(std::ios_base::failbit);         // silence the library's progress chatter
		w->m_scene.load_scene("", "", work, gltf);
		std::cout.clear();
		w->m_should_terminate = false;
		w->m_completed_rays = 0;
		w->resolution = fvec2((float)X, (float)Y);          // as worker::run sets it (worker.cpp:36-38)
		w->sample_count = spp;
		w->bounce_count = (uint8_t)bounces;
		g_worker = w.get();
		moodycamel::on_empty = queue_ran_dry;
	}
	~rig() { g_worker = nullptr; moodycamel::on_empty = nullptr; }

	template <typename F> void stage(F f, uint32_t* k_stream) {
		const unsigned before = g_seed_calls;
		w->m_should_terminate = false;
		((*w).*f)();
		if (g_seed_calls != before) {
			if (!k_stream || *k_stream != 0xFFFFFFFFu || g_seed_calls != before + 1) throw std::runtime_error("unexpected mt19937 seeding");
			*k_stream = before;
		}
	}
	bool busy() const {
		return w->m_object_intersection_queue.size_approx() || w->m_object_intersection_result_queue.size_approx() ||
		       w->m_direct_lighting_intersection_queue.size_approx() || w->m_direct_lighting_intersection_result_queue.size_approx() ||
		       w->m_shading_queue.size_approx();
	}
	// one sample through the pipeline, alone
	models::cloud_ray run(const models::cloud_ray& in) {
		using W = processors::worker;
		if (busy() || w->m_accumulate_queue.size_approx()) throw std::runtime_error("queues are not empty");
		w->m_object_intersection_queue.enqueue(in);
		while (busy()) {
			stage(&W::process_object_intersections, &k_sun);
			stage(&W::process_object_intersection_results, nullptr);
			stage(&W::process_direct_lighting_intersections, nullptr);
			stage(&W::process_direct_lighting_intersection_results, nullptr);
			stage(&W::process_shading, &k_shading);
		}
		models::cloud_ray out{};
		if (w->m_accumulate_queue.size_approx() != 1 || !w->m_accumulate_queue.try_dequeue(out)) throw std::runtime_error("no finished ray");
		if (out.uuid != in.uuid) throw std::runtime_error("uuid changed");
		return out;
	}
	std::vector<uint32_t> meta(uint32_t X, uint32_t Y, uint32_t spp, uint32_t bounces) const {
		return {seed_base(), k_jitter, k_sun, k_shading, X, Y, spp, bounces};
	}
};

static void push_result(std::vector<float>& rays, std::vector<float>& out, const geometry::ray& r, const models::cloud_ray& done) {
	push3(rays, r.origin); push3(rays, r.get_dir());
	push3(out, done.color); out.push_back(done.alpha);
}

static int cmd_frame(const char* gltf, const std::string& dir, uint32_t X, uint32_t Y, uint32_t spp, uint32_t bounces) {
	rig g(gltf, parse_work(gltf, 0, nullptr, 0), X, Y, spp, bounces);
	std::filesystem::create_directories(dir);
	const unsigned before = g_seed_calls;
	g.w->generate_rays();                                 // worker.cpp:114-149, as it is
	if (g_seed_calls != before) g.k_jitter = before;
	std::vector<models::cloud_ray> todo;
	for (models::cloud_ray r{}; g.w->m_object_intersection_queue.size_approx() && g.w->m_object_intersection_queue.try_dequeue(r);) todo.push_back(r);
	std::vector<uint64_t> uuid;
	std::vector<float> rays, out;
	for (const auto& r : todo) {
		const geometry::ray cam = r.ray;
		const models::cloud_ray done = g.run(r);
		uuid.push_back(r.uuid);
		push_result(rays, out, cam, done);
	}
	save(dir, "wf_uuid", uuid);
	save(dir, "wf_rays", rays, {todo.size(), 6}); save(dir, "wf_out", out, {todo.size(), 4});
	save(dir, "wf_meta", g.meta(X, Y, spp, bounces));
	return 0;
}

static int cmd_trace(const char* gltf, const std::string& dir, uint64_t seed, size_t n, uint32_t bounces) {
	rig g(gltf, parse_work(gltf, 0, nullptr, 0), 640, 480, 1, bounces);
	std::filesystem::create_directories(dir);
	fvec3 wmin(1e30f), wmax(-1e30f);
	for (auto& m : visit_order(g.w->m_scene)) {
		const scene::transform& t = m.ent->get_global_transform();
		for (int k = 0; k < 8; k++) {
			fvec3 c((k & 1) ? m.model->aabb.max.x : m.model->aabb.min.x, (k & 2) ? m.model->aabb.max.y : m.model->aabb.min.y,
			        (k & 4) ? m.model->aabb.max.z : m.model->aabb.min.z);
			fvec3 w = t * c;
			wmin = math::min(wmin, w); wmax = math::max(wmax, w);
		}
	}
	auto cam = g.w->m_scene.m_camera->get_component<scene::camera>();
	const fvec3 eye = g.w->m_scene.m_camera->get_global_transform().origin;
	pcg32 gen(seed);
	std::vector<float> rays, out;
	for (size_t i = 0; i < n; i++) {
		geometry::ray ray = (i & 1) ? geometry::ray(eye, normalize(wmin + (wmax - wmin) * gen.vec(0.05f, 0.95f) - eye))
		                            : cam->get_ray(fvec2(gen.range(-1, 1), gen.range(-1, 1)), 16.f / 9.f);
		models::cloud_ray cr{};                             // filled as generate_rays fills it (worker.cpp:137-143)
		cr.uuid = i;
		cr.ray = ray;
		cr.color = fvec4::zero;
		cr.scale = fvec3::one;
		cr.bounce = g.w->bounce_count;
		cr.stage = models::ray_stage::INTERSECT;
		push_result(rays, out, ray, g.run(cr));
	}
	save(dir, "wt_rays", rays, {n, 6}); save(dir, "wt_out", out, {n, 4});
	save(dir, "wt_meta", g.meta(640, 480, 1, bounces));
	return 0;
}

static int cmd_scene(const char* gltf, const std::string& dir, int argc, char** argv, int first) {
	rig g(gltf, parse_work(gltf, argc, argv, first), 640, 480, 1, 1);
	std::filesystem::create_directories(dir);
	const cloud::distributed_scene& sc = g.w->m_scene;
	auto models = visit_order(sc);
	std::vector<float> xf, verts, mats;
	std::vector<int32_t> model_surf, surf_rng;
	std::vector<uint32_t> tris;
	std::vector<uint8_t> mat_tex;
	std::string names;
	int32_t nsurf = 0;
	std::map<const core::material*, int32_t> mat_id;
	for (auto& m : models) {
		const scene::transform& t = m.ent->get_global_transform();
		push3(xf, t.origin); push3(xf, t.basis.x); push3(xf, t.basis.y); push3(xf, t.basis.z);
		model_surf.push_back(nsurf); model_surf.push_back((int32_t)m.model->surfaces.size());
		names += m.ent->get_name() + "\n";
		for (auto& s : m.model->surfaces) {
			mat_id[s.material.get()] = nsurf++;
			int32_t v0 = (int32_t)(verts.size() / 11), t0 = (int32_t)(tris.size() / 3);
			for (auto& v : s.mesh->vertices) {
				push3(verts, v.position); verts.push_back(v.tex_coord.x); verts.push_back(v.tex_coord.y);
				push3(verts, v.normal); push3(verts, v.tangent);
			}
			for (auto& tr : s.mesh->triangles) { tris.push_back(tr.x); tris.push_back(tr.y); tris.push_back(tr.z); }
			surf_rng.insert(surf_rng.end(), {v0, (int32_t)s.mesh->vertices.size(), t0, (int32_t)s.mesh->triangles.size()});
			auto& mt = *s.material;
			push3(mats, mt.albedo_fac); mats.push_back(mt.opacity_fac); mats.push_back(mt.roughness_fac);
			mats.push_back(mt.metallic_fac); push3(mats, mt.emissive_fac); mats.push_back(mt.ior);
			mats.push_back(mt.shadow_catcher ? 1.f : 0.f);
			mat_tex.insert(mat_tex.end(), {(uint8_t)!!mt.normal_tex, (uint8_t)!!mt.albedo_tex, (uint8_t)!!mt.opacity_tex,
			                               (uint8_t)!!mt.occlusion_tex, (uint8_t)!!mt.roughness_tex,
			                               (uint8_t)!!mt.metallic_tex, (uint8_t)!!mt.emissive_tex});
		}
	}
	save(dir, "model_xform", xf, {models.size(), 12});
	save(dir, "model_surf", model_surf, {models.size(), 2});
	save(dir, "surf_range", surf_rng, {(size_t)nsurf, 4});
	save(dir, "vertices", verts, {verts.size() / 11, 11});
	save(dir, "triangles", tris, {tris.size() / 3, 3});
	save(dir, "materials", mats, {(size_t)nsurf, 11});
	save(dir, "material_tex", mat_tex, {(size_t)nsurf, 7});
	std::vector<uint8_t> nm(names.begin(), names.end());
	save(dir, "model_names", nm);
	auto cam = sc.m_camera->get_component<scene::camera>();
	const scene::transform& ct = sc.m_camera->get_global_transform();
	std::vector<float> camv;
	push3(camv, ct.origin); push3(camv, ct.basis.x); push3(camv, ct.basis.y); push3(camv, ct.basis.z);
	camv.push_back(cam->get_fov()); camv.push_back(math::tan(cam->get_fov() * 0.5F));
	save(dir, "camera", camv);
	std::vector<float> sun;
	if (sc.m_sun_light) {
		const scene::transform& st = sc.m_sun_light->get_global_transform();
		auto sl = sc.m_sun_light->get_component<scene::sun_light>();
		push3(sun, st.basis.x); push3(sun, st.basis.y); push3(sun, st.basis.z);
		push3(sun, sl->energy); sun.push_back(sl->angular_radius);
	}
	save(dir, "sun", sun);

	// a stored ray batch through both of the scene's queries (src/scene/intersect.cpp:9-79, :82-151)
	fvec3 wmin(1e30f), wmax(-1e30f);
	for (auto& m : models) {
		if (m.model->surfaces.empty()) continue;
		const scene::transform& t = m.ent->get_global_transform();
		for (int k = 0; k < 8; k++) {
			fvec3 c((k & 1) ? m.model->aabb.max.x : m.model->aabb.min.x, (k & 2) ? m.model->aabb.max.y : m.model->aabb.min.y,
			        (k & 4) ? m.model->aabb.max.z : m.model->aabb.min.z);
			fvec3 w = t * c;
			wmin = math::min(wmin, w); wmax = math::max(wmax, w);
		}
	}
	const fvec3 eye = ct.origin;
	pcg32 gen(20240607);
	const size_t n = 600;
	std::vector<float> rays, out, mn;
	std::vector<int32_t> idx;
	for (size_t i = 0; i < n; i++) {
		geometry::ray ray = (i % 3 == 0) ? cam->get_ray(fvec2(gen.range(-1, 1), gen.range(-1, 1)), 16.f / 9.f)
		                  : (i % 3 == 1) ? geometry::ray(eye, normalize(wmin + (wmax - wmin) * gen.vec(0.05f, 0.95f) - eye))
		                                 : geometry::ray(wmin + (wmax - wmin) * gen.vec(-0.2f, 1.2f), normalize(gen.vec(-1, 1) + fvec3(0, 1e-3f, 0)));
		push3(rays, ray.origin); push3(rays, ray.get_dir());
		auto res = sc.intersect(ray);
		auto rm = sc.intersect_min_result(ray);
		idx.push_back(res.hit ? mat_id[res.material.get()] : -1);
		if (res.hit) {
			push3(out, res.position); out.push_back(res.tex_coord.x); out.push_back(res.tex_coord.y);
			push3(out, res.normal); push3(out, res.tangent); push3(out, res.get_normal());
		} else for (int k = 0; k < 14; k++) out.push_back(0);
		mn.push_back(rm.hit ? 1.f : 0.f); mn.push_back(rm.distance);
		if (rm.hit) { push3(mn, rm.position); push3(mn, rm.normal); } else for (int k = 0; k < 6; k++) mn.push_back(0);
	}
	save(dir, "ws_rays", rays, {n, 6}); save(dir, "ws_out", out, {n, 14}); save(dir, "ws_idx", idx); save(dir, "ws_min", mn, {n, 8});
	return 0;
}

int main(int argc, char** argv) {
	std::string cmd = argc > 1 ? argv[1] : "";
	try {
		if (cmd == "worker-frame" && argc == 8) return cmd_frame(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));
		if (cmd == "worker-trace" && argc == 7) return cmd_trace(argv[2], argv[3], strtoull(argv[4], 0, 10), strtoull(argv[5], 0, 10), atoi(argv[6]));
		if (cmd == "worker-scene" && argc >= 4) return cmd_scene(argv[2], argv[3], argc, argv, 4);
	} catch (const std::exception& e) {
		fprintf(stderr, "host_harness: %s\n", e.what());
		return 2;
	}
	fprintf(stderr, "usage: host_harness worker-frame|worker-trace|worker-scene ... (see header comment)\n");
	return 1;
}
