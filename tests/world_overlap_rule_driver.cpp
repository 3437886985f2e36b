// world_overlap_rule_driver.cpp -- rtk_amd/csrc/rtk_world_overlap_rule.h on the CPU (tests/test_world_overlap_cpu.py builds this
// with the host compiler, -ffp-contract=off as the library is built, plain and under the address and undefined-behaviour
// sanitizers, against the rule headers alone).
//
// Reads cases from the file named on the command line, one per line, every number as the hexadecimal bits of a 32-bit word unless
// said otherwise:
//     s T  followed by 9 T words               a scene of T triangle records (T decimal); scenes are numbered as they come
//     i scene allowed m0 .. m11                an instance (scene and allowed decimal; allowed: live and let through by the mask)
//     q shape ignore flags room  w ...         shape: b (6 words: lo, hi), o (15: centre, half, axes), t (9: three vertices).
//                                              ignore (hexadecimal): the instance left out; flags: the touching calls'; room
//                                              decimal, -1: all. BRUTE FORCE over (instance, record) in ascending order
//                                              through rtk_world_overlap_insert. Prints: count, then (instance prim) per kept entry
//     w shape ignore flags seed  w ...         the same answer (room: all) by THE WALK of a two-level hierarchy made here: per
//                                              instance the proxy box (rtk_world_box of the scene's root box) as it is, then the
//                                              scene's root box and its leaves of four records, local boxes, through
//                                              rtk_world_overlap_skip under the placement; the records of every scene are dealt
//                                              to leaves, and instances and leaves visited, in an order shuffled by seed (decimal;
//                                              0: as they come). Prints what q prints
//     n room K  followed by K pairs hi lo      rtk_world_overlap_insert of K keys in this order into a segment of `room` entries
//                                              inside a buffer of room + 4 entries of 0x7e bytes. Prints: kept, then the whole
//                                              buffer as (hi lo) pairs
// one line of output per q, w and n, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_world_overlap_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

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

// 24 bits of a 64-bit linear congruential generator
struct Gen {
	uint64_t s;
	uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 40); }
};

template <class T>
static void shuffle(std::vector<T> &v, Gen &g)
{
	for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[g.next() % i]);
}

struct Instance { uint32_t scene, allowed; float m[12]; };

// a query of one of the three shapes: its liveness, its bounds, and its candidate rule on placed vertices
struct Query {
	char shape;
	uint32_t flags;
	bool live;
	float lo[3], hi[3];                    // the bounds every skip compares against
	float c[3], h[3];                      // box
	rtk_obb_prepared obb;
	rtk_touch_hoist hoist;
	float a[3][3];                         // triangle

	bool prepare(char s, const float *w, uint32_t f)
	{
		shape = s; flags = f;
		if (s == 'b') {
			for (int k = 0; k < 3; k++) { lo[k] = w[k]; hi[k] = w[3 + k]; }
			rtk_box_centre(lo, hi, c, h);
			live = rtk_box_live(lo, hi);
		} else if (s == 'o') {
			live = rtk_obb_prepare(w, obb);
			for (int k = 0; k < 3; k++) { lo[k] = obb.qlo[k]; hi[k] = obb.qhi[k]; }
		} else if (s == 't') {
			for (int k = 0; k < 9; k++) a[k / 3][k % 3] = w[k];
			rtk_touch_hoist_query(a[0], a[1], a[2], hoist);
			live = rtk_touch_live(a[0], a[1], a[2]);
			for (int k = 0; k < 3; k++) { lo[k] = hoist.lo[k]; hi[k] = hoist.hi[k]; }
		} else return false;
		return true;
	}
	bool candidate(const float *v0, const float *v1, const float *v2, uint32_t prim) const
	{
		if (!live) return false;
		if (shape == 'b') return rtk_box_candidate(v0, v1, v2, lo, hi, c, h);
		if (shape == 'o') return rtk_obb_candidate(obb, live, v0, v1, v2);
		return rtk_touch_candidate(hoist, a[0], a[1], a[2], v0, v1, v2, prim, 0u, flags);
	}
};

static int floats_of(char shape) { return shape == 'b' ? 6 : shape == 'o' ? 15 : shape == 't' ? 9 : -1; }

static void print_entries(uint32_t count, const std::vector<uint64_t> &seg, uint32_t kept)
{
	printf("%" PRIx32, count);
	for (uint32_t k = 0; k < kept; k++) printf(" %" PRIx32 " %" PRIx32, (uint32_t)(seg[k] >> 32), (uint32_t)seg[k]);
	printf("\n");
}

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "world_overlap_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<std::vector<float>> scenes;
	std::vector<Instance> instances;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		bool ok = true;
		if (kind == 's') {
			unsigned long T;
			ok = fscanf(in, "%lu", &T) == 1;
			std::vector<float> t(ok ? 9 * T : 0);
			ok = ok && read_words(in, (int)(9 * T), t.data());
			scenes.push_back(t);
		} else if (kind == 'i') {
			Instance x;
			ok = fscanf(in, "%" SCNu32 " %" SCNu32, &x.scene, &x.allowed) == 2 && read_words(in, 12, x.m) && x.scene < scenes.size();
			instances.push_back(x);
		} else if (kind == 'q' || kind == 'w') {
			char shape;
			uint32_t ignore, flags;
			long long last;                                           // room (q) or seed (w)
			float w[15];
			ok = fscanf(in, " %c %" SCNx32 " %" SCNx32 " %lld", &shape, &ignore, &flags, &last) == 4 && floats_of(shape) > 0 && read_words(in, floats_of(shape), w);
			Query Q;
			ok = ok && Q.prepare(shape, w, flags);
			if (ok && kind == 'q') {
				// the count first, then the segment
				uint32_t count = 0;
				std::vector<uint64_t> keys;
				for (uint32_t i = 0; i < instances.size(); i++) {
					const Instance &x = instances[i];
					if (!x.allowed || i == ignore) continue;
					const std::vector<float> &t = scenes[x.scene];
					for (uint32_t prim = 0; prim < t.size() / 9; prim++) {
						float v0[3], v1[3], v2[3];
						rtk_world_overlap_place(x.m, &t[9 * prim], &t[9 * prim + 3], &t[9 * prim + 6], v0, v1, v2);
						if (Q.candidate(v0, v1, v2, prim)) { count++; keys.push_back(rtk_world_overlap_key(i, prim)); }
					}
				}
				const uint32_t room = last < 0 ? count : (uint32_t)last;
				std::vector<uint64_t> seg(room + 1u, 0ull);
				uint32_t kept = 0;
				uint64_t worst = 0;
				for (uint64_t key : keys) kept = rtk_world_overlap_insert(seg.data(), room, kept, key, worst);
				print_entries(count, seg, kept);
			} else if (ok) {
				Gen g = { (uint64_t)last };
				std::vector<uint32_t> order(instances.size());
				for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
				if (last) shuffle(order, g);
				uint32_t count = 0, kept = 0;
				uint64_t worst = 0;
				std::vector<uint64_t> seg;
				// (room: all. The segment is grown ahead of every insert, so that it is never full)
				for (uint32_t i : order) {
					const Instance &x = instances[i];
					if (!x.allowed || i == ignore || !Q.live) continue;
					const std::vector<float> &t = scenes[x.scene];
					const uint32_t T = (uint32_t)(t.size() / 9);
					if (T == 0) continue;
					std::vector<uint32_t> recs(T);
					for (uint32_t k = 0; k < T; k++) recs[k] = k;
					if (last) shuffle(recs, g);
					// the local boxes: leaves of four records, and the root over all of them
					const uint32_t L = (T + 3u) / 4u;
					std::vector<float> llo(3 * L), lhi(3 * L);
					float rlo[3] = { 0.0f, 0.0f, 0.0f }, rhi[3] = { 0.0f, 0.0f, 0.0f };
					for (uint32_t k = 0; k < T; k++) {
						for (int v = 0; v < 3; v++) {
							for (int a = 0; a < 3; a++) {
								const float c = t[9 * recs[k] + 3 * v + a];
								float &lo = llo[3 * (k / 4) + a], &hi = lhi[3 * (k / 4) + a];
								if ((k % 4 == 0 && v == 0) || c < lo) lo = c;
								if ((k % 4 == 0 && v == 0) || c > hi) hi = c;
								if ((k == 0 && v == 0) || c < rlo[a]) rlo[a] = c;
								if ((k == 0 && v == 0) || c > rhi[a]) rhi[a] = c;
							}
						}
					}
					// the proxy as it is; then the scene's boxes under the placement
					float plo[3], phi[3];
					if (!rtk_world_box(rlo, rhi, x.m, plo, phi)) continue;    // (a box that is not finite: a dead instance)
					if (rtk_world_overlap_skip(nullptr, plo, phi, Q.lo, Q.hi)) continue;
					if (rtk_world_overlap_skip(x.m, rlo, rhi, Q.lo, Q.hi)) continue;
					std::vector<uint32_t> leaves(L);
					for (uint32_t l = 0; l < L; l++) leaves[l] = l;
					if (last) shuffle(leaves, g);
					for (uint32_t l : leaves) {
						if (rtk_world_overlap_skip(x.m, &llo[3 * l], &lhi[3 * l], Q.lo, Q.hi)) continue;
						for (uint32_t k = 4 * l; k < 4 * l + 4 && k < T; k++) {
							const uint32_t prim = recs[k];
							float v0[3], v1[3], v2[3];
							rtk_world_overlap_place(x.m, &t[9 * prim], &t[9 * prim + 3], &t[9 * prim + 6], v0, v1, v2);
							if (!Q.candidate(v0, v1, v2, prim)) continue;
							count++;
							seg.resize(count + 1u, 0ull);
							kept = rtk_world_overlap_insert(seg.data(), count, kept, rtk_world_overlap_key(i, prim), worst);
						}
					}
				}
				print_entries(count, seg, kept);
			}
		} else if (kind == 'n') {
			unsigned long room, K;
			ok = fscanf(in, "%lu %lu", &room, &K) == 2;
			std::vector<uint64_t> buf(room + 4u);
			memset(buf.data(), 0x7e, buf.size() * sizeof(uint64_t));
			uint32_t kept = 0;
			uint64_t worst = 0;
			for (unsigned long k = 0; ok && k < K; k++) {
				uint32_t hi, lo;
				ok = fscanf(in, "%" SCNx32 " %" SCNx32, &hi, &lo) == 2;
				if (ok) kept = rtk_world_overlap_insert(buf.data(), (uint32_t)room, kept, ((uint64_t)hi << 32) | lo, worst);
			}
			if (ok) {
				printf("%" PRIx32, kept);
				for (uint64_t e : buf) printf(" %" PRIx32 " %" PRIx32, (uint32_t)(e >> 32), (uint32_t)e);
				printf("\n");
			}
		} else ok = false;
		if (!ok) { fprintf(stderr, "world_overlap_rule_driver: case %lu: cannot read a '%c' line\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
