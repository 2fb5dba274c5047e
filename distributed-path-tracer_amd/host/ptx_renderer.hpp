// Host-side C++ mirror of the reference's renderer interface (core::renderer,
// path-tracer-core/path_tracer_lib/path_tracer/core/renderer.hpp:15-36) over the C ABI of include/ptx.h:
// same public field names and defaults, load_gltf(path), render() -> PNG bytes, exceptions for errors
// (renderer.cpp:73-74,97-98 throw std::runtime_error). This is the binding a maintainer of the reference adds;
// see INTEGRATION.md. Header-only; link with libptx_hip.so.
#pragma once
#include <ptx.h>

#include <cstdint>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace core {

class renderer {
public:
	static constexpr uint32_t no_sun_light = 0xFFFFFFFFu;   // renderer.hpp:19

	struct uvec2 { uint32_t x, y; };
	uvec2 resolution{1920, 1080};          // renderer.hpp:21
	uint32_t thread_count = 0;             // kept for source compatibility; the GPU grid replaces util::thread_pool
	uint32_t sample_count = 10000;
	uint8_t bounce_count = 4;
	std::filesystem::path environment;     // PNG environment map (the reference holds a loaded image::texture, renderer.hpp:28); empty = none
	float environment_factor[3] = {1, 1, 1};
	bool transparent_background = false;   // renderer.cpp:340-399, :444: alpha 0 where trace() returns a miss, claim blend over the samples (ptx_render_transparent)
	uint32_t camera_index = 0;
	uint32_t sun_light_index = 0;
	uint8_t visualize_kd_tree_depth = 0;   // not built: mesh.cpp:316-318 colours each KD node by its heap address, nothing reproducible to mirror
	uint64_t seed = 0x5EED;                // key of the counter-based RNG (the reference seeds from random_device)
	uint32_t nee_candidates = 1;           // render_nee and its kin: the light sample is picked among this many candidates, 1 .. 16 (PTX_NEE_CANDIDATES)
	// render_adaptive (no counterpart in the reference): the threshold of the stopping rule, the samples every pixel gets first and the samples
	// per further round (0 = adaptive_min); sample_count is the cap
	float adaptive_threshold = 0.1f;
	uint32_t adaptive_min = 8, adaptive_step = 0;
	// thin lens of the loaded camera (ptx_scene_set_camera; no counterpart in the reference), applied before a render: circumradius of the
	// aperture (0 = the pinhole), distance of the plane of focus, corners of the aperture polygon (0 = 16), angle of corner 0
	float lens_radius = 0, focus_distance = 0;
	uint32_t blades = 0;
	float blade_rotation = 0;
	// render_denoised, render_adaptive(denoise) and render_adaptive_nee(denoise): the first-hit emission of the guides' samples
	// (ptx_render_emission) is taken out of the halves before the filter and added to its output (ptx_emission_split, ptx_emission_merge)
	bool split_emission = false;

	explicit renderer(int device = 0) { check(ptx_ctx_create(device, &ctx_)); }
	renderer(const renderer&) = delete;
	renderer& operator=(const renderer&) = delete;
	~renderer() {
		ptx_scene_destroy(scene_);
		ptx_ctx_destroy(ctx_);
	}

	void load_gltf(const std::filesystem::path& path) {
		ptx_load_opts o{camera_index, sun_light_index};
		ptx_scene_destroy(scene_);
		scene_ = nullptr;
		env_set_.clear();
		lens_set_ = lens{};
		check(ptx_scene_load_gltf(ctx_, path.string().c_str(), &o, &scene_));
	}
	// the lens fields onto the loaded camera, when they changed since the last render
	void apply_lens() const {
		const lens want{lens_radius, focus_distance, blades, blade_rotation};
		if (want.radius == lens_set_.radius && want.focus == lens_set_.focus && want.blades == lens_set_.blades && want.rotation == lens_set_.rotation) return;
		ptx_camera cam{};
		check(ptx_scene_get_camera(scene_, &cam));
		cam.lens_radius = lens_radius; cam.focus_distance = focus_distance; cam.blades = blades; cam.blade_rotation = blade_rotation;
		check(ptx_scene_set_camera(scene_, &cam));
		lens_set_ = want;
	}

	// The `point` and `spot` lights of a glTF file (KHR_lights_punctual) as 16-float records (ptx_gltf_read_punctual_lights; include/ptx.h has
	// the record). Host only.
	static std::vector<float> read_punctual_lights(const std::filesystem::path& path) {
		const int64_t n = ptx_gltf_read_punctual_lights(path.string().c_str(), nullptr, 0);
		if (n < 0) throw std::runtime_error(ptx_last_error());
		std::vector<float> recs((size_t)n * 16);
		if (n && ptx_gltf_read_punctual_lights(path.string().c_str(), recs.data(), recs.size()) < 0) throw std::runtime_error(ptx_last_error());
		return recs;
	}
	// Point and spot lights for render_nee and its kin, which sample them as a third strategy (ptx_scene_set_punctual_lights); render() and the
	// other calls ignore them. An empty vector removes them.
	void set_punctual_lights(const std::vector<float>& records) {
		if (!scene_) throw std::runtime_error("set_punctual_lights() before load_gltf()");
		if (records.size() % 16) throw std::runtime_error("set_punctual_lights: the records are 16 floats each");
		check(ptx_scene_set_punctual_lights(scene_, records.empty() ? nullptr : records.data(), (uint32_t)(records.size() / 16)));
	}
	// How a punctual sample picks its light (ptx_scene_set_punctual_pick): PTX_PUNCTUAL_PICK_CDF, the default, or PTX_PUNCTUAL_PICK_TREE, a
	// light tree descended from the shading point. The mode survives set_punctual_lights.
	void set_punctual_pick(uint32_t pick) {
		if (!scene_) throw std::runtime_error("set_punctual_pick() before load_gltf()");
		check(ptx_scene_set_punctual_pick(scene_, pick));
	}
	uint32_t punctual_pick() const {
		if (!scene_) throw std::runtime_error("punctual_pick() before load_gltf()");
		uint32_t pick = 0;
		check(ptx_scene_get_punctual_pick(scene_, &pick));
		return pick;
	}
	// How a light sample picks its emissive triangle (ptx_scene_set_light_pick): PTX_LIGHT_PICK_CDF, the default, or PTX_LIGHT_PICK_TREE, a
	// light tree over the light list descended from the shading point. The mode outlives the light list.
	void set_light_pick(uint32_t pick) {
		if (!scene_) throw std::runtime_error("set_light_pick() before load_gltf()");
		check(ptx_scene_set_light_pick(scene_, pick));
	}
	uint32_t light_pick() const {
		if (!scene_) throw std::runtime_error("light_pick() before load_gltf()");
		uint32_t pick = 0;
		check(ptx_scene_get_light_pick(scene_, &pick));
		return pick;
	}
	// The stochastic pick alone for n (position, u) records of 4 floats, host memory (ptx_light_pick_batch) -> the list entries; pmf receives
	// their probabilities
	std::vector<int32_t> light_pick_batch(const std::vector<float>& pos_u, std::vector<float>& pmf) const {
		if (!scene_) throw std::runtime_error("light_pick_batch() before load_gltf()");
		if (pos_u.size() % 4) throw std::runtime_error("light_pick_batch: the records are 4 floats each");
		std::vector<int32_t> light(pos_u.size() / 4);
		pmf.assign(light.size(), 0.0f);
		check(ptx_light_pick_batch(scene_, pos_u.data(), light.size(), light.data(), pmf.data()));
		return light;
	}
	// pmf_k(x) for n positions of 3 floats and n list entries, host memory (ptx_light_pmf_batch)
	std::vector<float> light_pmf_batch(const std::vector<float>& pos, const std::vector<int32_t>& light) const {
		if (!scene_) throw std::runtime_error("light_pmf_batch() before load_gltf()");
		if (pos.size() != 3 * light.size()) throw std::runtime_error("light_pmf_batch: three floats per entry");
		std::vector<float> pmf(light.size(), 0.0f);
		check(ptx_light_pmf_batch(scene_, pos.data(), light.data(), light.size(), pmf.data()));
		return pmf;
	}
	// The pick alone for n (position, u) records of 4 floats, host memory (ptx_punctual_pick_batch) -> the lights; pmf receives their probabilities
	std::vector<int32_t> punctual_pick_batch(const std::vector<float>& pos_u, std::vector<float>& pmf) const {
		if (!scene_) throw std::runtime_error("punctual_pick_batch() before load_gltf()");
		if (pos_u.size() % 4) throw std::runtime_error("punctual_pick_batch: the records are 4 floats each");
		std::vector<int32_t> light(pos_u.size() / 4);
		pmf.assign(light.size(), 0.0f);
		check(ptx_punctual_pick_batch(scene_, pos_u.data(), light.size(), light.data(), pmf.data()));
		return light;
	}

	// radiance sums [H][W][4]; with transparent_background set: the blended means (colour, alpha) of ptx_render_transparent. stats optional
	std::vector<float> render_accum(ptx_render_stats* stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render() before load_gltf()");
		if (visualize_kd_tree_depth) throw std::runtime_error("visualize_kd_tree_depth is not built: the reference colours KD nodes by their heap addresses (mesh.cpp:316-318)");
		apply_lens();
		if (environment.string() != env_set_) {   // (re)load the map only when the field changed
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		std::vector<float> accum((size_t)c.W * c.H * 4, 0.f);
		if (transparent_background) {
			std::vector<uint8_t> claimed((size_t)c.W * c.H, 0);
			check(ptx_render_transparent(scene_, &c, accum.data(), claimed.data(), stats));
		} else {
			check(ptx_render(scene_, &c, accum.data(), stats));
		}
		return accum;
	}

	// Guide buffers of the frame's camera samples for a denoiser (ptx_render_aov): SUMS over sample_count samples, [H][W][4] each —
	// albedo rgb + coverage count, world shading normal xyz + depth sum. Divide by the coverage count for means. stats optional
	struct aov { std::vector<float> albedo_cov, normal_depth; };
	aov render_aov(ptx_render_stats* stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_aov() before load_gltf()");
		apply_lens();
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count;
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		aov a{std::vector<float>((size_t)c.W * c.H * 4, 0.f), std::vector<float>((size_t)c.W * c.H * 4, 0.f)};
		const ptx_aov_buffers b{a.albedo_cov.data(), a.normal_depth.data()};
		check(ptx_render_aov(scene_, &c, &b, stats));
		return a;
	}

	// First-hit emission SUMS of the frame's sample_count camera samples (ptx_render_emission), [H][W][4]: emissive * 10 of every sample's
	// surface that faces the camera + the count of those samples. stats optional
	std::vector<float> render_emission(ptx_render_stats* stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_emission() before load_gltf()");
		apply_lens();
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count;
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		std::vector<float> emission((size_t)c.W * c.H * 4, 0.f);
		check(ptx_render_emission(scene_, &c, emission.data(), stats));
		return emission;
	}
	// ptx_emission_split / ptx_emission_merge on host buffers of [..][4] floats: emission SUMS over guide_spp samples of every pixel out of the
	// radiance sums a and b (b may be nullptr) before a filter call, and back into the MEANS it returned
	void emission_split(const std::vector<float>& emission, uint32_t guide_spp, std::vector<float>& a, std::vector<float>* b = nullptr) const {
		if (a.size() != emission.size() || (b && b->size() != emission.size())) throw std::runtime_error("emission_split: the buffers differ in size");
		check(ptx_emission_split(ctx_, emission.data(), guide_spp, emission.size() / 4, a.data(), b ? b->data() : nullptr));
	}
	void emission_merge(const std::vector<float>& emission, uint32_t guide_spp, std::vector<float>& out) const {
		if (out.size() != emission.size()) throw std::runtime_error("emission_merge: the buffers differ in size");
		check(ptx_emission_merge(ctx_, emission.data(), guide_spp, emission.size() / 4, out.data()));
	}

	// The frame through the variance-guided a-trous filter (ptx_denoise): samples [0, n/2) and [n/2, n) of sample_count = n rendered into two
	// buffers, the guide buffers of all n; returns the filtered MEANS [H][W][4] (write them with ptx_tonemap_encode(..., spp = 1)). stats optional
	std::vector<float> render_denoised(ptx_denoise_stats* stats = nullptr, const ptx_denoise_cfg* filter = nullptr) const {
		if (!scene_) throw std::runtime_error("render_denoised() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_denoised: the filter takes radiance sums, which transparent_background does not produce");
		if (sample_count < 2) throw std::runtime_error("render_denoised: sample_count must be at least 2 (the noise estimate needs two half-frames)");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		const size_t floats = (size_t)c.W * c.H * 4;
		std::vector<float> a(floats, 0.f), b(floats, 0.f), alb(floats, 0.f), nd(floats, 0.f);
		c.spp = sample_count / 2;
		check(ptx_render(scene_, &c, a.data(), nullptr));
		c.sample0 = c.spp; c.spp = sample_count - c.sample0;
		check(ptx_render(scene_, &c, b.data(), nullptr));
		c.sample0 = 0; c.spp = sample_count;
		const ptx_aov_buffers g{alb.data(), nd.data()};
		check(ptx_render_aov(scene_, &c, &g, nullptr));
		ptx_denoise_cfg d = filter ? *filter : ptx_denoise_cfg{};   // iterations and sigmas; the rest is set here
		d.W = c.W; d.H = c.H; d.spp_a = sample_count / 2; d.spp_b = sample_count - d.spp_a;
		std::vector<float> em;
		if (split_emission) {
			em.assign(floats, 0.f);
			check(ptx_render_emission(scene_, &c, em.data(), nullptr));
			emission_split(em, sample_count, a, &b);
		}
		check(ptx_denoise(ctx_, &d, a.data(), b.data(), &g, a.data(), stats));
		if (split_emission) emission_merge(em, sample_count, a);
		return a;
	}

	// The frame with noise-driven per-pixel sample counts (ptx_render_adaptive; sample_count is the cap): returns the MEANS [H][W][4] (write them
	// with ptx_tonemap_encode(..., spp = 1)). stats optional: render.samples / (W * H) is the mean count. denoise: the frame through the filter
	// (ptx_denoise_counts on the guides of the first adaptive_min samples, which every pixel has); dstats optional
	std::vector<float> render_adaptive(ptx_adaptive_stats* stats = nullptr, bool denoise = false, ptx_denoise_stats* dstats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_adaptive() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_adaptive: the decision takes radiance sums, which transparent_background does not produce");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		const ptx_adaptive_cfg ac{adaptive_min, adaptive_step, adaptive_threshold};
		const size_t floats = (size_t)c.W * c.H * 4;
		std::vector<float> a(floats, 0.f), b(floats, 0.f);
		check(ptx_render_adaptive(scene_, &c, &ac, a.data(), b.data(), stats));
		return adaptive_frame(c, a, b, denoise, dstats);
	}

	// The adaptive frame over several processes, interleaved tiles (ptx_ctx_set_mask_exchange in include/ptx.h has the loop): the exchange
	// that merges the ranks' noisy bytes after every round. mask: the caller's buffer of at least W * H bytes, host or device memory; fn ==
	// nullptr clears the registration. The callback runs inside render_adaptive_shard and must not call this renderer; one that enqueues its
	// collective (ncclAllReduce(mask, mask, n, ncclUint8, ncclMax, comm, stream)) takes stream() beforehand.
	void set_mask_exchange(ptx_mask_exchange_fn fn, void* user, uint8_t* mask, size_t mask_bytes) { check(ptx_ctx_set_mask_exchange(ctx_, fn, user, mask, mask_bytes)); }
	void* stream() const { return ptx_ctx_stream(ctx_); }
	// Rank `index` of `count`'s share of render_adaptive's frame (tile: the shard tile's side, 0 = 64): ADDS the radiance sums of its own
	// pixels to the half-buffers a and b ([H][W][4], zero-initialised by the caller; host or device memory) and leaves the others untouched.
	// The sum of the ranks' buffers is bitwise the one-process frame's halves: reduce them onto the root, then ptx_accum_mean or
	// ptx_denoise_counts there. nee_flags: nullptr = ptx_render_adaptive, else ptx_render_adaptive_nee with those flags.
	void render_adaptive_shard(uint32_t index, uint32_t count, uint32_t tile, float* a, float* b, const uint32_t* nee_flags = nullptr, ptx_adaptive_stats* stats = nullptr,
	                           ptx_adaptive_nee_stats* nee_stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_adaptive_shard() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_adaptive_shard: the decision takes radiance sums, which transparent_background does not produce");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		c.shard_index = index; c.shard_count = count; c.shard_tile = tile;
		const ptx_adaptive_cfg ac{adaptive_min, adaptive_step, adaptive_threshold};
		if (nee_flags) {
			ptx_nee_cfg n{};
			n.flags = *nee_flags;
			check(ptx_render_adaptive_nee(scene_, &c, &ac, &n, a, b, nee_stats));
		} else {
			check(ptx_render_adaptive(scene_, &c, &ac, a, b, stats));
		}
	}

	// render_adaptive on render_nee's estimator (ptx_render_adaptive_nee; flags: ptx_nee_cfg::flags): one sequence of passes per round, resolved
	// into both halves. Returns the MEANS [H][W][4], through the filter with denoise. stats, dstats optional
	std::vector<float> render_adaptive_nee(ptx_adaptive_nee_stats* stats = nullptr, uint32_t flags = 0, bool denoise = false, ptx_denoise_stats* dstats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_adaptive_nee() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_adaptive_nee: the decision takes radiance sums, which transparent_background does not produce");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		const ptx_adaptive_cfg ac{adaptive_min, adaptive_step, adaptive_threshold};
		const ptx_nee_cfg n{flags | nee_bits()};
		const size_t floats = (size_t)c.W * c.H * 4;
		std::vector<float> a(floats, 0.f), b(floats, 0.f);
		check(ptx_render_adaptive_nee(scene_, &c, &ac, &n, a.data(), b.data(), stats));
		return adaptive_frame(c, a, b, denoise, dstats);
	}

	// The light-sampled frame through the filter (ptx_denoise): samples [0, n/2) and [n/2, n) of sample_count = n rendered with ptx_render_nee
	// into two buffers, the guide buffers of all n; returns the filtered MEANS [H][W][4]. stats optional
	std::vector<float> render_nee_denoised(uint32_t flags = 0, ptx_denoise_stats* stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_nee_denoised() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_nee_denoised: transparent_background's blend is not built on this estimator");
		if (sample_count < 2) throw std::runtime_error("render_nee_denoised: sample_count must be at least 2 (the noise estimate needs two half-frames)");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		const size_t floats = (size_t)c.W * c.H * 4;
		std::vector<float> a(floats, 0.f), b(floats, 0.f), alb(floats, 0.f), nd(floats, 0.f);
		const ptx_nee_cfg n{flags | nee_bits()};
		c.spp = sample_count / 2;
		check(ptx_render_nee(scene_, &c, &n, a.data(), nullptr));
		c.sample0 = c.spp; c.spp = sample_count - c.sample0;
		check(ptx_render_nee(scene_, &c, &n, b.data(), nullptr));
		c.sample0 = 0; c.spp = sample_count;
		const ptx_aov_buffers g{alb.data(), nd.data()};
		check(ptx_render_aov(scene_, &c, &g, nullptr));
		ptx_denoise_cfg d{};
		d.W = c.W; d.H = c.H; d.spp_a = sample_count / 2; d.spp_b = sample_count - d.spp_a;
		check(ptx_denoise(ctx_, &d, a.data(), b.data(), &g, a.data(), stats));
		return a;
	}

	// Per-pixel motion SUMS of the frame's sample_count camera samples against the previous frame (ptx_render_motion), [H][W][4]: previous minus
	// current screen position, distance from the previous camera, 1. prev_camera: the camera one frame earlier (nullptr: it did not move);
	// prev_model_xform: the [n_models][12] transforms one frame earlier (nullptr or empty: no model moved). stats optional
	std::vector<float> render_motion(const ptx_camera* prev_camera = nullptr, const std::vector<float>* prev_model_xform = nullptr, ptx_render_stats* stats = nullptr) const {
		if (!scene_) throw std::runtime_error("render_motion() before load_gltf()");
		apply_lens();
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count;
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		std::vector<float> motion((size_t)c.W * c.H * 4, 0.f);
		const bool xf = prev_model_xform && !prev_model_xform->empty();
		const ptx_motion_prev prev{prev_camera, xf ? prev_model_xform->data() : nullptr, xf ? (uint32_t)(prev_model_xform->size() / 12) : 0u};
		check(ptx_render_motion(scene_, &c, (prev_camera || xf) ? &prev : nullptr, motion.data(), stats));
		return motion;
	}
	// the loaded camera as stored, and the model transforms in PTX_ARR_MODEL_XFORM's layout: what a caller keeps as "one frame earlier"
	ptx_camera camera() const {
		if (!scene_) throw std::runtime_error("camera() before load_gltf()");
		ptx_camera cam{};
		check(ptx_scene_get_camera(scene_, &cam));
		return cam;
	}
	std::vector<float> model_xforms() const {
		if (!scene_) throw std::runtime_error("model_xforms() before load_gltf()");
		const int64_t n = ptx_scene_get_array(scene_, PTX_ARR_MODEL_XFORM, nullptr, 0);
		if (n < 0) throw std::runtime_error(ptx_last_error());
		std::vector<float> x((size_t)n);
		if (n && ptx_scene_get_array(scene_, PTX_ARR_MODEL_XFORM, x.data(), x.size() * sizeof(float)) != n) throw std::runtime_error(ptx_last_error());
		return x;
	}

	// An animation through ptx_denoise_temporal (or, after set_adaptive, ptx_denoise_temporal_counts): owns the two ping-ponged histories and
	// the previous frame's camera and model transforms.
	// frame() moves the scene (optionally), renders the two half-frames, the guides and the motion against the previous frame, accumulates and
	// filters, and returns the filtered MEANS [H][W][4]. Frame k is rendered with the key seed + k, so that the frames' noise is independent.
	// A change of resolution starts the history over. The renderer must outlive the sequence.
	class temporal_sequence {
	public:
		explicit temporal_sequence(renderer& r) : r_(r) {}
		ptx_temporal_cfg filter{};   // iterations, sigmas, max_history, taus (0 = the defaults); W, H and the sample counts are set per frame
		uint32_t frames() const { return frames_; }
		void restart() { have_ = false; }
		// camera: the frame's pose (origin, basis, yfov; the lens stays the renderer's fields), nullptr = where it is; model_xform: the frame's
		// [n_models][12] transforms, nullptr = where they are. stats optional
		std::vector<float> frame(const ptx_camera* camera = nullptr, const std::vector<float>* model_xform = nullptr, ptx_temporal_stats* stats = nullptr) {
			if (!r_.scene_) throw std::runtime_error("temporal_sequence::frame() before load_gltf()");
			if (r_.transparent_background) throw std::runtime_error("temporal_sequence: the filter takes radiance sums, which transparent_background does not produce");
			if (r_.sample_count < 2) throw std::runtime_error("temporal_sequence: sample_count must be at least 2 (the noise estimate needs two half-frames)");
			if (camera) {
				ptx_camera cam = *camera;
				cam.lens_radius = r_.lens_radius; cam.focus_distance = r_.focus_distance; cam.blades = r_.blades; cam.blade_rotation = r_.blade_rotation;
				check(ptx_scene_set_camera(r_.scene_, &cam));
				r_.lens_set_ = lens{r_.lens_radius, r_.focus_distance, r_.blades, r_.blade_rotation};
			} else {
				r_.apply_lens();
			}
			if (model_xform) check(ptx_scene_set_model_xforms(r_.scene_, model_xform->data(), (uint32_t)(model_xform->size() / 12)));
			if (r_.environment.string() != r_.env_set_) {
				check(ptx_scene_set_environment(r_.scene_, r_.environment.empty() ? nullptr : r_.environment.string().c_str(), 1));
				r_.env_set_ = r_.environment.string();
			}
			const uint32_t W = r_.resolution.x, H = r_.resolution.y, n = r_.sample_count;
			const size_t px = (size_t)W * H;
			if (W != w_ || H != h_) {
				have_ = false; w_ = W; h_ = H;
				for (history& h : hist_) { h.color.assign(px * 4, 0.f); h.moments.assign(px * 2, 0.f); h.geometry.assign(px * 4, 0.f); }
			}
			ptx_render_cfg c{};
			c.W = W; c.H = H; c.bounces = r_.bounce_count;
			for (int k = 0; k < 3; k++) c.env[k] = r_.environment_factor[k];
			const uint64_t key = r_.seed + frames_;
			c.seed_lo = (uint32_t)key; c.seed_hi = (uint32_t)(key >> 32);
			std::vector<float> a(px * 4, 0.f), b(px * 4, 0.f), alb(px * 4, 0.f), nd(px * 4, 0.f), motion(px * 4, 0.f), out(px * 4, 0.f);
			history &hp = hist_[cur_], &hn = hist_[cur_ ^ 1u];
			const ptx_temporal_history prev{hp.color.data(), hp.moments.data(), hp.geometry.data()}, next{hn.color.data(), hn.moments.data(), hn.geometry.data()};
			const ptx_aov_buffers g{alb.data(), nd.data()};
			const ptx_motion_prev mp{&prev_cam_, prev_xf_.empty() ? nullptr : prev_xf_.data(), (uint32_t)(prev_xf_.size() / 12)};
			if (adaptive_) {
				// the halves with per-pixel counts (sample_count is the cap), the guides and the motion over the min_spp samples every pixel has
				c.spp = n;
				const ptx_adaptive_cfg ac{ad_min_, ad_step_, ad_threshold_};
				if (ad_nee_) {
					const ptx_nee_cfg nc{ad_nee_flags_ | r_.nee_bits()};
					check(ptx_render_adaptive_nee(r_.scene_, &c, &ac, &nc, a.data(), b.data(), nullptr));
				} else {
					check(ptx_render_adaptive(r_.scene_, &c, &ac, a.data(), b.data(), nullptr));
				}
				c.spp = ad_min_;
				check(ptx_render_aov(r_.scene_, &c, &g, nullptr));
				check(ptx_render_motion(r_.scene_, &c, have_ ? &mp : nullptr, motion.data(), nullptr));
				const std::vector<float> em = split(c, ad_min_, a, b);
				ptx_temporal_counts_cfg t{};
				t.W = W; t.H = H; t.guide_spp = ad_min_; t.iterations = filter.iterations;
				t.sigma_l = filter.sigma_l; t.sigma_n = filter.sigma_n; t.sigma_z = filter.sigma_z;
				t.max_history = filter.max_history; t.tau_z = filter.tau_z; t.tau_n = filter.tau_n; t.flags = ad_temporal_flags_;
				check(ptx_denoise_temporal_counts(r_.ctx_, &t, a.data(), b.data(), &g, motion.data(), have_ ? &prev : nullptr, &next, out.data(), stats));
				if (split_) r_.emission_merge(em, ad_min_, out);
				return finish(out);
			}
			c.spp = n / 2;
			check(ptx_render(r_.scene_, &c, a.data(), nullptr));
			c.sample0 = c.spp; c.spp = n - c.sample0;
			check(ptx_render(r_.scene_, &c, b.data(), nullptr));
			c.sample0 = 0; c.spp = n;
			check(ptx_render_aov(r_.scene_, &c, &g, nullptr));
			check(ptx_render_motion(r_.scene_, &c, have_ ? &mp : nullptr, motion.data(), nullptr));
			const std::vector<float> em = split(c, n, a, b);
			ptx_temporal_cfg t = filter;
			t.W = W; t.H = H; t.spp_a = n / 2; t.spp_b = n - n / 2;
			check(ptx_denoise_temporal(r_.ctx_, &t, a.data(), b.data(), &g, motion.data(), have_ ? &prev : nullptr, &next, out.data(), stats));
			if (split_) r_.emission_merge(em, n, out);
			return finish(out);
		}
		// Adaptive frames (ptx_denoise_temporal_counts): frame() renders the halves with ptx_render_adaptive, or with ptx_render_adaptive_nee when
		// nee_flags is given (ptx_nee_cfg::flags, to which the renderer's nee_candidates adds its bits), the renderer's sample_count being the
		// cap; the guides and the motion over the first min_spp samples; and keeps a history counted in samples: filter.max_history is then in
		// samples. temporal_flags: PTX_TEMPORAL_*. The two kinds of history do not mix: the call starts the history over.
		void set_adaptive(uint32_t min_spp, uint32_t step_spp, float threshold, const uint32_t* nee_flags = nullptr, uint32_t temporal_flags = 0) {
			adaptive_ = true;
			ad_min_ = min_spp; ad_step_ = step_spp; ad_threshold_ = threshold;
			ad_nee_ = nee_flags != nullptr;
			ad_nee_flags_ = nee_flags ? *nee_flags : 0u;
			ad_temporal_flags_ = temporal_flags;
			have_ = false;
		}
		// The first-hit emission of the guides' samples goes round the temporal call: split before it, merged after it. The history then holds
		// the residual, which does not mix with a history built without the split: a change starts the history over.
		void set_split_emission(bool on) {
			if (on != split_) have_ = false;
			split_ = on;
		}
		// this frame's history: integrated demodulated colour + history length, luminance moments, mean normal + depth
		const std::vector<float>& history_color() const { return hist_[cur_].color; }

	private:
		struct history { std::vector<float> color, moments, geometry; };
		// the frame is in `next`: swap the histories and remember the scene's state as "one frame earlier"
		std::vector<float> finish(std::vector<float>& out) {
			cur_ ^= 1u;
			have_ = true;
			frames_++;
			prev_cam_ = r_.camera();
			prev_xf_ = r_.model_xforms();
			return std::move(out);
		}
		// with the split on: the emission sums of the guides' samples (c as the guides were rendered with), taken out of the halves
		std::vector<float> split(const ptx_render_cfg& c, uint32_t guide_spp, std::vector<float>& a, std::vector<float>& b) const {
			std::vector<float> em;
			if (!split_) return em;
			em.assign(a.size(), 0.f);
			check(ptx_render_emission(r_.scene_, &c, em.data(), nullptr));
			r_.emission_split(em, guide_spp, a, &b);
			return em;
		}
		bool adaptive_ = false, ad_nee_ = false, split_ = false;
		uint32_t ad_min_ = 0, ad_step_ = 0, ad_nee_flags_ = 0, ad_temporal_flags_ = 0;
		float ad_threshold_ = 0;
		renderer& r_;
		history hist_[2];
		uint32_t cur_ = 0, w_ = 0, h_ = 0, frames_ = 0;
		bool have_ = false;
		ptx_camera prev_cam_{};
		std::vector<float> prev_xf_;
	};

	// nee_candidates as the bits of ptx_nee_cfg::flags
	uint32_t nee_bits() const {
		if (nee_candidates < 1 || nee_candidates > 16) throw std::runtime_error("nee_candidates must be 1 .. 16");
		return PTX_NEE_CANDIDATES(nee_candidates);
	}

	// Radiance sums [H][W][4] of the frame with next-event estimation towards the scene's emissive triangles (ptx_render_nee): render_accum()'s
	// samples plus one MIS-weighted light sample per continuing vertex; the same expectation, less noise where emitters light the scene.
	// Write them with encode(sums, sample_count). stats optional; flags: ptx_nee_cfg::flags (PTX_NEE_FUSED: the same frame from one kernel launch per pass;
	// PTX_NEE_ENV_SAMPLES: the light sample may go towards `environment` too; PTX_NEE_SAMPLER_PDF: MIS weights on the density of LIB's BSDF sampler),
	// to which nee_candidates adds its bits
	std::vector<float> render_nee(ptx_nee_stats* stats = nullptr, uint32_t flags = 0) const {
		if (!scene_) throw std::runtime_error("render_nee() before load_gltf()");
		if (transparent_background) throw std::runtime_error("render_nee: transparent_background's blend is not built on this estimator");
		apply_lens();
		if (environment.string() != env_set_) {
			check(ptx_scene_set_environment(scene_, environment.empty() ? nullptr : environment.string().c_str(), 1));
			env_set_ = environment.string();
		}
		ptx_render_cfg c{};
		c.W = resolution.x; c.H = resolution.y; c.spp = sample_count; c.bounces = bounce_count;
		for (int k = 0; k < 3; k++) c.env[k] = environment_factor[k];
		c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
		std::vector<float> accum((size_t)c.W * c.H * 4, 0.f);
		const ptx_nee_cfg n{flags | nee_bits()};
		check(ptx_render_nee(scene_, &c, &n, accum.data(), stats));
		return accum;
	}

	std::vector<uint8_t> render() const {   // renderer.cpp:334-428: PNG bytes (RGBA8, ACES tonemap, sRGB)
		return encode(render_accum(), transparent_background ? 1u : sample_count);
	}
	// the same image write for a buffer of sums over `spp` samples; the transparent mode's and the filter's means are written as they are
	// (spp = 1: x / 1.0f is exact)
	std::vector<uint8_t> encode(const std::vector<float>& accum, uint32_t spp) const {
		std::vector<uint8_t> rgba((size_t)resolution.x * resolution.y * 4);
		check(ptx_tonemap_encode(ctx_, accum.data(), resolution.x, resolution.y, spp, rgba.data()));
		uint8_t* png = nullptr;
		size_t n = 0;
		check(ptx_encode_png(rgba.data(), resolution.x, resolution.y, &png, &n));
		std::vector<uint8_t> out(png, png + n);
		ptx_free(png);
		return out;
	}

private:
	// the means of two adaptive half-buffers, or the halves through ptx_denoise_counts with the guides of the first adaptive_min samples
	std::vector<float> adaptive_frame(ptx_render_cfg c, std::vector<float>& a, std::vector<float>& b, bool denoise, ptx_denoise_stats* dstats) const {
		if (!denoise) {
			check(ptx_accum_mean(ctx_, a.data(), b.data(), a.size() / 4, a.data()));
			return std::move(a);
		}
		std::vector<float> alb(a.size(), 0.f), nd(a.size(), 0.f);
		const ptx_aov_buffers g{alb.data(), nd.data()};
		c.spp = adaptive_min;
		check(ptx_render_aov(scene_, &c, &g, nullptr));
		ptx_denoise_counts_cfg d{};
		d.W = c.W; d.H = c.H; d.guide_spp = adaptive_min;
		std::vector<float> em;
		if (split_emission) {
			em.assign(a.size(), 0.f);
			check(ptx_render_emission(scene_, &c, em.data(), nullptr));
			emission_split(em, adaptive_min, a, &b);
		}
		check(ptx_denoise_counts(ctx_, &d, a.data(), b.data(), &g, a.data(), dstats));
		if (split_emission) emission_merge(em, adaptive_min, a);
		return std::move(a);
	}
	static void check(int rc) {
		if (rc != PTX_OK) throw std::runtime_error(std::string(ptx_last_error()));
	}
	ptx_ctx* ctx_ = nullptr;
	ptx_scene* scene_ = nullptr;
	mutable std::string env_set_;
	struct lens { float radius = 0, focus = 0; uint32_t blades = 0; float rotation = 0; };
	mutable lens lens_set_;
};

}  // namespace core
