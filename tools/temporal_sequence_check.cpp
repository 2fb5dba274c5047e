// Drives core::renderer::temporal_sequence and core::renderer::render_motion (host/ptx_renderer.hpp), the C++ mirror of
// ptx_denoise_temporal and ptx_render_motion, for tests/test_temporal_gpu.py, which compares what it writes with the Python mirror's frames.
//   temporal_sequence_check SCENE.gltf W H SPP BOUNCES POSES.bin OUT.bin [MIN:STEP:THRESHOLD:NEE_FLAGS:TEMPORAL_FLAGS | -] [split]
// The optional argument makes the sequence adaptive (temporal_sequence::set_adaptive; tests/test_temporal_counts_gpu.py): SPP is then the cap,
// NEE_FLAGS = - renders with ptx_render_adaptive, a number with ptx_render_adaptive_nee and those flags.
// A second optional argument, the word split, keeps first-hit emission out of the temporal call (temporal_sequence::set_split_emission;
// tests/test_emission_gpu.py); a uniform sequence with the split takes - as the first.
// POSES.bin: one camera per frame, 13 float32 each (origin, basis columns, yfov). OUT.bin receives, as float32: per frame the filtered
// means [H][W][4]; then the last frame's integrated colour [H][W][4]; then render_motion of the last frame against the first camera.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../distributed-path-tracer_amd/host/ptx_renderer.hpp"

int main(int argc, char** argv) {
	if (argc < 8 || argc > 10 || (argc == 10 && strcmp(argv[9], "split"))) {
		fprintf(stderr, "usage: %s SCENE.gltf W H SPP BOUNCES POSES.bin OUT.bin [MIN:STEP:THRESHOLD:NEE_FLAGS:TEMPORAL_FLAGS | -] [split]\n", argv[0]);
		return 2;
	}
	try {
		std::vector<float> poses;
		if (FILE* f = fopen(argv[6], "rb")) {
			float v[13];
			while (fread(v, sizeof v, 1, f) == 1) poses.insert(poses.end(), v, v + 13);
			fclose(f);
		}
		if (poses.empty()) { fprintf(stderr, "no poses in %s\n", argv[6]); return 2; }
		core::renderer r(0);
		r.resolution = {(uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3])};
		r.sample_count = (uint32_t)atoi(argv[4]);
		r.bounce_count = (uint8_t)atoi(argv[5]);
		r.load_gltf(argv[1]);
		auto camera_of = [&](size_t k) {
			ptx_camera c{};
			memcpy(c.origin, &poses[13 * k], 12);
			memcpy(c.basis, &poses[13 * k + 3], 36);
			c.yfov = poses[13 * k + 12];
			return c;
		};
		FILE* out = fopen(argv[7], "wb");
		if (!out) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
		core::renderer::temporal_sequence seq(r);
		if (argc == 10) seq.set_split_emission(true);
		if (argc >= 9 && strcmp(argv[8], "-")) {
			unsigned min_spp = 0, step_spp = 0, temporal_flags = 0;
			float threshold = 0;
			char nee[32] = "";
			if (sscanf(argv[8], "%u:%u:%f:%31[^:]:%u", &min_spp, &step_spp, &threshold, nee, &temporal_flags) != 5) { fprintf(stderr, "bad adaptive argument %s\n", argv[8]); return 2; }
			const uint32_t nee_flags = (uint32_t)strtoul(nee, nullptr, 0);
			seq.set_adaptive(min_spp, step_spp, threshold, strcmp(nee, "-") ? &nee_flags : nullptr, temporal_flags);
		}
		for (size_t k = 0; k < poses.size() / 13; k++) {
			const ptx_camera c = camera_of(k);
			ptx_temporal_stats st{};
			const std::vector<float> frame = seq.frame(&c, nullptr, &st);
			fwrite(frame.data(), sizeof(float), frame.size(), out);
			printf("frame %zu: accumulate %.4f ms, filter %.4f ms, reprojected %llu, reset %llu\n", k, st.accumulate_ms, st.filter.kernel_ms,
			       (unsigned long long)st.reprojected, (unsigned long long)st.reset);
		}
		fwrite(seq.history_color().data(), sizeof(float), seq.history_color().size(), out);
		const ptx_camera first = camera_of(0);
		const std::vector<float> xf = r.model_xforms();
		const std::vector<float> motion = r.render_motion(&first, &xf);
		fwrite(motion.data(), sizeof(float), motion.size(), out);
		fclose(out);
	} catch (const std::exception& e) {
		fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
	return 0;
}
