// Minimal C++ host over the mirror class: what path-tracer-core/src/main.cpp + worker.cpp reduce to once the
// Lambda / S3 plumbing (out of scope) is taken away:
//   ptx_render_cli [--transparent] [--denoise] [--split-emission] [--nee] [--nee-fused] [--nee-env MAP] [--nee-sampler-pdf] [--nee-candidates M] [--nee-punctual] [--nee-punctual-tree] [--nee-light-tree] [--adaptive THR[:MIN[:STEP]]] [--lens R:F[:BLADES[:ROT]]] [--aov PREFIX] <scene.gltf> <out.png> [W H spp bounces]
//       --transparent: renderer::transparent_background
//       --denoise:     writes the frame through the variance-guided a-trous filter (renderer::render_denoised) in place of the plain one
//       --split-emission: with --denoise, alone or with --adaptive (with or without --nee*): the first-hit emission of the guides' samples is
//                      taken out of the half-frames before the filter and added, unfiltered, to its output (renderer::split_emission);
//                      an error without --denoise and with --nee --denoise, whose half-frames renderer::render_nee_denoised filters as they are
//       --nee:         light sampling towards the scene's emissive triangles (renderer::render_nee)
//       --nee-fused:   --nee with one kernel launch per pass (PTX_NEE_FUSED): the same frame; ignored on scenes of the queue pipeline
//       --nee-env MAP: --nee under the environment map MAP (renderer::environment; PNG, JPEG or Radiance .hdr), the light sample going
//                      towards the map too (PTX_NEE_ENV_SAMPLES); combines with --nee-fused
//       --nee-sampler-pdf: --nee with the MIS weights built on the density of the BSDF sampler (PTX_NEE_SAMPLER_PDF): the frame's expectation
//                      is the plain renderer's at glossy vertices too; combines with --nee-fused, --nee-env and --adaptive
//       --nee-candidates M: --nee with the light sample of a vertex picked among M = 1 .. 16 candidates, still one shadow ray
//                      (PTX_NEE_CANDIDATES); combines with --nee-fused, --nee-env, --nee-sampler-pdf and --adaptive
//       --adaptive THR[:MIN[:STEP]]: noise-driven per-pixel sample counts (renderer::render_adaptive) with spp as the cap: every pixel gets MIN
//                      samples (8), then rounds of STEP (MIN) go to the pixels whose half-frames still disagree by more than THR
//       --nee-punctual: with --nee (or a switch that implies it): the `point` and `spot` lights of the glTF being rendered (KHR_lights_punctual)
//                      are read and set on the scene, and the light sample takes them as a third strategy; without --nee it is an error
//       --nee-punctual-tree: --nee-punctual with the light of a punctual sample picked from a light tree by its distance from the shading point
//                      (renderer::set_punctual_pick, PTX_PUNCTUAL_PICK_TREE) instead of by intensity alone; implies --nee-punctual
//       --nee-light-tree: implies --nee: the emissive triangle of a light sample is picked from a light tree over the light list by its power and
//                      distance from the shading point (renderer::set_light_pick, PTX_LIGHT_PICK_TREE) instead of by area alone. Combines
//                      with every other --nee switch; with --nee-fused the fused kernel's tree variants render
//       combinations:  --adaptive with --nee / --nee-fused / --nee-env / --nee-sampler-pdf / --nee-candidates renders the adaptive loop on the light-sampling estimator
//                      (renderer::render_adaptive_nee); --adaptive --denoise, with or without --nee*, filters the adaptive frame
//                      (ptx_denoise_counts on the guides of the first MIN samples); --nee* --denoise filters two light-sampled half-frames
//                      (renderer::render_nee_denoised). --transparent combines with none of them
//       --lens R:F[:BLADES[:ROT]]: a thin lens on the loaded camera (renderer::lens_radius ...): aperture circumradius R > 0 in scene units, focused
//                      at distance F > 0, the aperture a regular polygon of BLADES corners (3 .. 32, default 16) turned by ROT radians;
//                      combines with every other switch
//       --aov PREFIX:  also writes the denoiser's guide images PREFIX_albedo.png (mean albedo of the covered samples, alpha = coverage)
//                      and PREFIX_normal.png (mean shading normal * 0.5 + 0.5), quantised linearly to 8 bits
//   ptx_render_cli --event <event.json> <local scene root dir> <out.png>     (the worker's Lambda event, main.cpp:9-25)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ptx_renderer.hpp"

// plain linear 8-bit quantiser of a value in [0, 1]
static uint8_t quant8(float v) {
	v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
	return (uint8_t)(v * 255.f + 0.5f);
}

static void write_png(const std::string& path, const std::vector<uint8_t>& rgba, uint32_t W, uint32_t H) {
	uint8_t* png = nullptr;
	size_t n = 0;
	if (ptx_encode_png(rgba.data(), W, H, &png, &n) != PTX_OK) throw std::runtime_error(ptx_last_error());
	std::ofstream(path, std::ios::binary).write((const char*)png, (std::streamsize)n);
	ptx_free(png);
}

int main(int argc, char** argv) {
	bool split_emission = false;
	bool transparent = false, denoise = false, adaptive = false, nee = false, nee_fused = false, nee_sampler_pdf = false, nee_punctual = false, nee_punctual_tree = false, nee_light_tree = false;
	float ad_thr = 0.1f;
	unsigned ad_min = 8, ad_step = 0, nee_candidates = 1;
	std::string aov_prefix, nee_env;
	float lens_r = 0, lens_f = 0, lens_rot = 0;
	unsigned lens_blades = 0;
	for (;;) {   // leading switches
		if (argc > 1 && std::string(argv[1]) == "--transparent") { transparent = true; argv[1] = argv[0]; argv++; argc--; }
		else if (argc > 1 && std::string(argv[1]) == "--denoise") { denoise = true; argv[1] = argv[0]; argv++; argc--; }
		else if (argc > 1 && std::string(argv[1]) == "--split-emission") { split_emission = true; argv[1] = argv[0]; argv++; argc--; }
		else if (argc > 1 && std::string(argv[1]) == "--nee") { nee = true; argv[1] = argv[0]; argv++; argc--; }   // renderer::render_nee: light sampling
		else if (argc > 1 && std::string(argv[1]) == "--nee-fused") { nee = nee_fused = true; argv[1] = argv[0]; argv++; argc--; }   // ... one launch per pass
		else if (argc > 1 && std::string(argv[1]) == "--nee-sampler-pdf") { nee = nee_sampler_pdf = true; argv[1] = argv[0]; argv++; argc--; }   // ... weights on the sampler's density
		else if (argc > 1 && std::string(argv[1]) == "--nee-punctual") { nee_punctual = true; argv[1] = argv[0]; argv++; argc--; }   // ... the file's point and spot lights too; does not imply --nee
		else if (argc > 1 && std::string(argv[1]) == "--nee-light-tree") { nee = nee_light_tree = true; argv[1] = argv[0]; argv++; argc--; }   // ... the triangle picked from the light tree
		else if (argc > 1 && std::string(argv[1]) == "--nee-punctual-tree") { nee_punctual = nee_punctual_tree = true; argv[1] = argv[0]; argv++; argc--; }   // ... picked from the light tree
		else if (argc > 2 && std::string(argv[1]) == "--nee-env") { nee = true; nee_env = argv[2]; argv[2] = argv[0]; argv += 2; argc -= 2; }   // ... the map as a light
		else if (argc > 2 && std::string(argv[1]) == "--nee-candidates") {   // ... picked among M candidates
			if (std::sscanf(argv[2], "%u", &nee_candidates) < 1 || nee_candidates < 1 || nee_candidates > 16) { std::fprintf(stderr, "error: --nee-candidates M, M = 1 .. 16\n"); return 1; }
			nee = true; argv[2] = argv[0]; argv += 2; argc -= 2;
		}
		else if (argc > 2 && std::string(argv[1]) == "--adaptive") {
			if (std::sscanf(argv[2], "%f:%u:%u", &ad_thr, &ad_min, &ad_step) < 1) { std::fprintf(stderr, "error: --adaptive THR[:MIN[:STEP]]\n"); return 1; }
			adaptive = true; argv[2] = argv[0]; argv += 2; argc -= 2;
		}
		else if (argc > 2 && std::string(argv[1]) == "--lens") {
			char tail = 0;
			const int got = std::sscanf(argv[2], "%f:%f:%u:%f%c", &lens_r, &lens_f, &lens_blades, &lens_rot, &tail);
			if (got < 2 || got > 4 || !(lens_r > 0) || !(lens_f > 0) || (got >= 3 && (lens_blades < 3 || lens_blades > 32))) {
				std::fprintf(stderr, "error: --lens R:F[:BLADES[:ROT]], R > 0, F > 0, BLADES = 3 .. 32\n");
				return 1;
			}
			argv[2] = argv[0]; argv += 2; argc -= 2;
		}
		else if (argc > 2 && std::string(argv[1]) == "--aov") { aov_prefix = argv[2]; argv[2] = argv[0]; argv += 2; argc -= 2; }
		else break;
	}
	if (argc < 3) {
		std::fprintf(stderr, "usage: %s [--transparent] [--denoise] [--split-emission] [--nee] [--nee-fused] [--nee-env MAP] [--nee-sampler-pdf] [--nee-candidates M] [--nee-punctual] [--nee-punctual-tree] [--nee-light-tree] [--adaptive THR[:MIN[:STEP]]] [--lens R:F[:BLADES[:ROT]]] [--aov PREFIX] <scene.gltf> <out.png> [W H spp bounces]\n", argv[0]);
		return 1;
	}
	if (nee_punctual && !nee) {
		std::fprintf(stderr, "error: --nee-punctual needs --nee (or --nee-fused, --nee-env, --nee-sampler-pdf, --nee-candidates): only the light-sampling estimator renders point and spot lights\n");
		return 1;
	}
	if (split_emission && (!denoise || (nee && !adaptive))) {
		std::fprintf(stderr, "error: --split-emission needs --denoise, alone or with --adaptive: it takes the first-hit emission round the filter\n");
		return 1;
	}
	if (argc == 5 && std::string(argv[1]) == "--event") {
		ptx_ctx* ctx = nullptr;
		ptx_scene* scene = nullptr;
		ptx_render_cfg cfg{};
		ptx_worker_event ev{};
		auto die = [&](const char* what) { std::fprintf(stderr, "error: %s: %s\n", what, ptx_last_error()); return 2; };
		if (ptx_ctx_create(0, &ctx) != PTX_OK) return die("ptx_ctx_create");
		if (ptx_worker_event_load(ctx, argv[2], argv[3], &scene, &cfg, &ev) != PTX_OK) return die("ptx_worker_event_load");
		std::vector<float> accum((size_t)cfg.W * cfg.H * 4, 0.f);
		ptx_render_stats st{};
		if (ptx_render(scene, &cfg, accum.data(), &st) != PTX_OK) return die("ptx_render");
		std::vector<uint8_t> rgba((size_t)cfg.W * cfg.H * 4);
		if (ptx_tonemap_encode(ctx, accum.data(), cfg.W, cfg.H, cfg.spp, rgba.data()) != PTX_OK) return die("ptx_tonemap_encode");
		uint8_t* png = nullptr;
		size_t n = 0;
		if (ptx_encode_png(rgba.data(), cfg.W, cfg.H, &png, &n) != PTX_OK) return die("ptx_encode_png");
		std::ofstream(argv[4], std::ios::binary).write((const char*)png, (std::streamsize)n);   // worker.cpp:101-104 uploads this as <scene_root>test.png
		ptx_free(png);
		std::printf("{\"worker_id\": \"%s\", \"num_workers\": %d, \"W\": %u, \"H\": %u, \"spp\": %u, \"bounces\": %u, \"rays\": %llu, \"kernel_ms\": %.3f}\n",
		            ev.worker_id, ev.num_workers, cfg.W, cfg.H, cfg.spp, cfg.bounces, (unsigned long long)st.rays, st.kernel_ms);
		ptx_scene_destroy(scene);
		ptx_ctx_destroy(ctx);
		return 0;
	}
	try {
		core::renderer r(0);
		r.transparent_background = transparent;
		if (argc >= 7) {
			r.resolution = {(uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4])};
			r.sample_count = (uint32_t)std::atoi(argv[5]);
			r.bounce_count = (uint8_t)std::atoi(argv[6]);
		} else {
			r.sample_count = 64;
		}
		r.load_gltf(argv[1]);
		if (!nee_env.empty()) r.environment = nee_env;
		r.nee_candidates = nee_candidates;
		r.split_emission = split_emission;
		r.lens_radius = lens_r; r.focus_distance = lens_f; r.blades = lens_blades; r.blade_rotation = lens_rot;
		if (nee_light_tree) r.set_light_pick(PTX_LIGHT_PICK_TREE);
		size_t n_punctual = 0;
		if (nee_punctual) {
			const std::vector<float> lamps = core::renderer::read_punctual_lights(argv[1]);
			r.set_punctual_lights(lamps);
			if (nee_punctual_tree) r.set_punctual_pick(PTX_PUNCTUAL_PICK_TREE);
			n_punctual = lamps.size() / 16;
		}
		auto t0 = std::chrono::steady_clock::now();
		ptx_denoise_stats dst{};
		ptx_adaptive_stats ast{};
		ptx_adaptive_nee_stats anst{};
		r.adaptive_threshold = ad_thr; r.adaptive_min = ad_min; r.adaptive_step = ad_step;
		ptx_nee_stats nst{};
		if (transparent && (nee || adaptive || denoise)) throw std::runtime_error("--transparent does not combine with --nee, --adaptive or --denoise");
		const uint32_t nee_flags = (nee_fused ? PTX_NEE_FUSED : 0u) | (nee_env.empty() ? 0u : PTX_NEE_ENV_SAMPLES) | (nee_sampler_pdf ? PTX_NEE_SAMPLER_PDF : 0u);
		std::vector<uint8_t> png;
		if (nee && adaptive) {
			png = r.encode(r.render_adaptive_nee(&anst, nee_flags, denoise, &dst), 1);
			nst = anst.nee;
			ast.render = anst.nee.render; ast.rounds = anst.rounds; ast.active_last = anst.active_last; ast.select_ms = anst.select_ms;
		} else if (nee) {
			png = denoise ? r.encode(r.render_nee_denoised(nee_flags, &dst), 1) : r.encode(r.render_nee(&nst, nee_flags), r.sample_count);
		} else if (adaptive) {
			png = r.encode(r.render_adaptive(&ast, denoise, &dst), 1);
		} else {
			png = denoise ? r.encode(r.render_denoised(&dst), 1) : r.render();
		}
		double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		std::ofstream(argv[2], std::ios::binary).write((const char*)png.data(), (std::streamsize)png.size());
		double aov_ms = 0;
		if (!aov_prefix.empty()) {
			ptx_render_stats st{};
			const core::renderer::aov a = r.render_aov(&st);
			aov_ms = st.kernel_ms;
			const uint32_t W = r.resolution.x, H = r.resolution.y;
			std::vector<uint8_t> alb((size_t)W * H * 4), nrm((size_t)W * H * 4);
			for (size_t p = 0; p < (size_t)W * H; p++) {
				const float cov = a.albedo_cov[4 * p + 3], inv = cov > 0.f ? 1.f / cov : 0.f;
				for (int k = 0; k < 3; k++) {
					alb[4 * p + k] = quant8(a.albedo_cov[4 * p + k] * inv);
					nrm[4 * p + k] = quant8(cov > 0.f ? a.normal_depth[4 * p + k] * inv * 0.5f + 0.5f : 0.f);
				}
				alb[4 * p + 3] = nrm[4 * p + 3] = quant8(cov / (float)r.sample_count);
			}
			write_png(aov_prefix + "_albedo.png", alb, W, H);
			write_png(aov_prefix + "_normal.png", nrm, W, H);
		}
		std::printf("{\"W\": %u, \"H\": %u, \"spp\": %u, \"bounces\": %u, \"seconds\": %.4f, \"png_bytes\": %zu", r.resolution.x, r.resolution.y,
		            r.sample_count, (unsigned)r.bounce_count, s, png.size());
		if (!aov_prefix.empty()) std::printf(", \"aov_kernel_ms\": %.3f", aov_ms);
		if (denoise) std::printf(", \"denoise_kernel_ms\": %.3f", dst.kernel_ms);
		if (adaptive)
			std::printf(", \"adaptive_mean_spp\": %.3f, \"adaptive_rounds\": %u, \"adaptive_active_last\": %u, \"adaptive_select_ms\": %.3f",
			            (double)ast.render.samples / ((double)r.resolution.x * r.resolution.y), ast.rounds, ast.active_last, ast.select_ms);
		if (nee && (adaptive || !denoise))   // the two half-frames of --nee --denoise are rendered without stats
			std::printf(", \"nee_lights\": %u, \"nee_light_samples\": %llu, \"nee_light_visible\": %llu, \"nee_kernel_ms\": %.3f", nst.n_lights,
			            (unsigned long long)nst.light_samples, (unsigned long long)nst.light_visible, nst.render.kernel_ms);
		if (nee_punctual) std::printf(", \"nee_punctual_lights\": %zu", n_punctual);
		if (nee_punctual_tree) std::printf(", \"nee_punctual_pick\": \"tree\"");
		if (nee_light_tree) std::printf(", \"nee_light_pick\": \"tree\"");
		std::printf("}\n");
	} catch (const std::exception& e) {
		std::fprintf(stderr, "error: %s\n", e.what());
		return 2;
	}
	return 0;
}
