// world_closest_rule_driver.cpp -- rtk_amd/csrc/rtk_world_closest_rule.h on the CPU (tests/test_world_closest_cpu.py builds this
// with the host compiler, -ffp-contract=off as the library is built, plain and under the address and undefined-behaviour
// sanitizers, against the rule headers alone).
//
// Reads cases from the file named on the command line, one per line, every number as the hexadecimal bits of a 32-bit word unless
// said otherwise:
//     b m0 .. m11 lo0 lo1 lo2 hi0 hi1 hi2      rtk_world_placed_box: prints wlo0 wlo1 wlo2 whi0 whi1 whi2
//     k m0 .. m11 lo0 lo1 lo2 hi0 hi1 hi2      min / max over the eight corners placed by rtk_place_vertex: prints the same six
//     c m0 .. m11 seed n scale                 containment under placement m, n rounds of the driver's own generator (seed and n
//                                              decimal, scale a float's bits: the size of the boxes): a random box, three random
//                                              points inside it, a random query. Prints: points placed outside the placed box, and
//                                              rounds where rtk_closest_box_bound(p, placed box) > dist2 of the placed triangle
//     s T  followed by 9 T words               a scene of T triangle records (T decimal); scenes are numbered as they come
//     i scene allowed m0 .. m11                an instance (scene and allowed decimal; allowed: live and let through by the mask)
//     q p0 p1 p2 max2 ignore                   the brute-force answer over all instances so far: prints dist2 u v prim inst q0 q1 q2
// one line of output per b, k, c and q, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_world_closest_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static bool read_words(FILE *in, int n, float *f, uint32_t *w = nullptr)
{
	for (int k = 0; k < n; k++) {
		uint32_t x;
		if (fscanf(in, "%" SCNx32, &x) != 1) return false;
		f[k] = as_float(x);
		if (w) w[k] = x;
	}
	return true;
}

// uniform in [0, 1): 24 bits of a 64-bit linear congruential generator
struct Gen {
	uint64_t s;
	float next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)(uint32_t)(s >> 40) * 0x1p-24f; }
};

struct Instance { uint32_t scene, allowed; float m[12]; };

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "world_closest_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<std::vector<float>> scenes;
	std::vector<Instance> instances;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		bool ok = true;
		if (kind == 'b' || kind == 'k') {
			float f[18], wlo[3], whi[3];
			ok = read_words(in, 18, f);
			if (ok && kind == 'b') rtk_world_placed_box(f, f + 12, f + 15, wlo, whi);
			else if (ok) {
				for (int c = 0; c < 8; c++) {
					float v[3] = { (c & 1) ? f[15] : f[12], (c & 2) ? f[16] : f[13], (c & 4) ? f[17] : f[14] };
					rtk_place_vertex(f, v[0], v[1], v[2]);
					for (int a = 0; a < 3; a++) {
						if (c == 0) { wlo[a] = whi[a] = v[a]; continue; }
						wlo[a] = v[a] < wlo[a] ? v[a] : wlo[a];
						whi[a] = v[a] > whi[a] ? v[a] : whi[a];
					}
				}
			}
			if (ok) printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", bits_of(wlo[0]), bits_of(wlo[1]), bits_of(wlo[2]),
				bits_of(whi[0]), bits_of(whi[1]), bits_of(whi[2]));
		} else if (kind == 'c') {
			float m[12], scale;
			unsigned long long seed, n;
			ok = read_words(in, 12, m) && fscanf(in, "%llu %llu", &seed, &n) == 2 && read_words(in, 1, &scale);
			unsigned long long outside = 0, above = 0;
			Gen g = { seed };
			for (unsigned long long r = 0; ok && r < n; r++) {
				// a box around a centre of up to 4 scales, with extents of 0 (every eighth axis) up to one scale
				float lo[3], hi[3], wlo[3], whi[3], tri[3][3], p[3];
				for (int a = 0; a < 3; a++) {
					const float c = (g.next() - 0.5f) * 8.0f * scale, e = g.next() < 0.125f ? 0.0f : g.next() * scale;
					lo[a] = c - e; hi[a] = c + e;
				}
				rtk_world_placed_box(m, lo, hi, wlo, whi);
				for (int v = 0; v < 3; v++) {
					for (int a = 0; a < 3; a++) {
						// (a corner coordinate now and then: the extremes must be inside too)
						const float t = g.next(), x = lo[a] + (hi[a] - lo[a]) * t;
						tri[v][a] = t < 0.05f ? lo[a] : t > 0.95f ? hi[a] : (x < lo[a] ? lo[a] : x > hi[a] ? hi[a] : x);
					}
					rtk_place_vertex(m, tri[v][0], tri[v][1], tri[v][2]);
					for (int a = 0; a < 3; a++) if (!(tri[v][a] >= wlo[a] && tri[v][a] <= whi[a])) outside++;
				}
				// a query from inside the placed box up to four of its sizes away
				for (int a = 0; a < 3; a++) p[a] = wlo[a] + (whi[a] - wlo[a]) * (g.next() * 9.0f - 4.0f);
				float q[3], u, v;
				int region;
				const float dist2 = rtk_closest_triangle(p, tri[0], tri[1], tri[2], q, u, v, region);
				const float bound = rtk_closest_box_bound(p, wlo, whi);
				if (!(bound <= dist2) && dist2 == dist2) above++;
			}
			if (ok) printf("%llu %llu\n", outside, above);
		} else if (kind == 's') {
			unsigned long T;
			ok = fscanf(in, "%lu", &T) == 1;
			std::vector<float> t(ok ? 9 * T : 0);
			ok = ok && read_words(in, (int)(9 * T), t.data());
			scenes.push_back(t);
		} else if (kind == 'i') {
			Instance x;
			ok = fscanf(in, "%" SCNu32 " %" SCNu32, &x.scene, &x.allowed) == 2 && read_words(in, 12, x.m) && x.scene < scenes.size();
			instances.push_back(x);
		} else if (kind == 'q') {
			float f[5];
			uint32_t w[5];
			ok = read_words(in, 5, f, w);
			if (ok) {
				// rtk_dev_closest_points's liveness: finite coordinates, a limit above zero (a NaN limit fails the comparison)
				const bool live = rtk_world_finite(f[0]) && rtk_world_finite(f[1]) && rtk_world_finite(f[2]) && f[3] > 0.0f;
				float best2 = f[3], bu = 0.0f, bv = 0.0f, bq[3] = { f[0], f[1], f[2] };
				uint32_t best_inst = 0xffffffffu, best_prim = 0xffffffffu;
				for (uint32_t i = 0; live && i < instances.size(); i++) {
					const Instance &x = instances[i];
					if (!x.allowed || i == w[4]) continue;
					const std::vector<float> &t = scenes[x.scene];
					for (uint32_t prim = 0; prim < t.size() / 9; prim++) {
						float q[3], u, v;
						const float dist2 = rtk_world_closest_triangle(f, x.m, &t[9 * prim], &t[9 * prim + 3], &t[9 * prim + 6], q, u, v);
						if (dist2 < f[3] && rtk_world_closest_better(dist2, i, prim, best2, best_inst, best_prim)) {
							best2 = dist2; best_inst = i; best_prim = prim; bu = u; bv = v;
							bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2];
						}
					}
				}
				const bool hit = best_prim != 0xffffffffu;
				printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n",
					hit ? bits_of(best2) : w[3], bits_of(bu), bits_of(bv), best_prim, best_inst, hit ? bits_of(bq[0]) : w[0], hit ? bits_of(bq[1]) : w[1],
					hit ? bits_of(bq[2]) : w[2]);
			}
		} else ok = false;
		if (!ok) { fprintf(stderr, "world_closest_rule_driver: case %lu: cannot read a '%c' line\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
