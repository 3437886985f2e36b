// Driver of tests/test_detect_rule_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_detect_rule.h alone (no HIP), with
// the address and undefined-behaviour sanitizers. argv[1] names a file of rtk_ray records (32 bytes each); the answer is one line,
// "w h": the image rtk_detect_host takes the batch for, or "0 0".
// On the way the step test of the header is compared, at every ray that has two neighbours, with the two forms it replaced: the
// ternaries the host had and the fmaxf arithmetic the device had, transcribed below. A difference ends the run with status 3.
#include "rtk_detect_rule.h"

#include <stdio.h>

#include <vector>

static bool step_jumps_ternaries(const rtk_ray *rays, size_t i)
{
	const float *a = reinterpret_cast<const float *>(rays + i - 1), *b = reinterpret_cast<const float *>(rays + i), *c = reinterpret_cast<const float *>(rays + i + 1);
	float m = 0.0f, dmax = 0.0f;
	for (int k = 0; k < 6; k++) {
		const float s0 = b[k] - a[k], s1 = c[k] - b[k];
		m = fabsf(s0) > m ? fabsf(s0) : m;
		dmax = fabsf(s1 - s0) > dmax ? fabsf(s1 - s0) : dmax;
	}
	return !(dmax <= 8.0f * m);
}

static bool step_jumps_fmaxf(const rtk_ray *rays, size_t i)
{
	const float *a = reinterpret_cast<const float *>(rays + i - 1), *b = reinterpret_cast<const float *>(rays + i), *c = reinterpret_cast<const float *>(rays + i + 1);
	float m = 0.0f, dmax = 0.0f;
	for (int k = 0; k < 6; k++) {
		const float s0 = b[k] - a[k], s1 = c[k] - b[k];
		m = fmaxf(m, fabsf(s0));
		dmax = fmaxf(dmax, fabsf(s1 - s0));
	}
	return !(dmax <= 8.0f * m);
}

int main(int argc, char **argv)
{
	if (argc != 2) return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	std::vector<rtk_ray> rays;
	rtk_ray r;
	while (fread(&r, sizeof(r), 1, f) == 1) rays.push_back(r);
	fclose(f);
	for (size_t i = 1; i + 1 < rays.size(); i++) {
		const bool rule = rtk_detect_step_jumps(rays.data(), i);
		if (rule != step_jumps_ternaries(rays.data(), i) || rule != step_jumps_fmaxf(rays.data(), i)) {
			fprintf(stderr, "the forms of the step test differ at ray %zu\n", i);
			return 3;
		}
	}
	uint32_t w = 1, h = 1;
	rtk_detect_host(rays.data(), rays.size(), &w, &h);
	printf("%u %u\n", w, h);
	return 0;
}
