// entries_rule_driver.cpp -- rtk_amd/csrc/rtk_entries_rule.h on the CPU (tests/test_entries_rule_cpu.py builds this with the host
// compiler, -ffp-contract=off and the address and undefined-behaviour sanitizers): the reduced-corner form of the beam's
// child test, which rtk_packet_entries_kernel runs, against the eight-product form it replaced -- the listed bound bit for
// bit and the admit decision -- on random beams and boxes and on the edge cases named below.
//
//   entries_rule_driver RANDOM_CASES SEED      prints "ok <edge cases> edge <random cases> random <cases the control differs in> control",
//                                              or the first mismatches, and exits 1 on any
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtk_entries_rule.h"

static uint64_t rng_state;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static float unit() { return (float)(rnd() >> 40) * 0x1p-24f; }                                   // [0, 1)
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float pow2(int e) { return ldexpf(1.0f, e); }

static unsigned long long cases, bad, control_bad;

// the control: the same two products per axis WITHOUT the select by the difference's sign -- it must differ somewhere, or the
// comparison below could not fail
static bool control_child(const float lo[3], const float hi[3], const RtkEntriesBeam &b, float *tlo)
{
	float n = b.tmin, f = INFINITY;
	for (int a = 0; a < 3; a++) {
		const bool neg = (b.neg >> a) & 1u;
		const float dn = (neg ? hi[a] : lo[a]) - (neg ? b.olo[a] : b.ohi[a]), df = (neg ? lo[a] : hi[a]) - (neg ? b.ohi[a] : b.olo[a]);
		n = fmaxf(n, dn * b.rlo[a] - b.m[a]);
		f = fminf(f, df * b.rhi[a] + b.m[a]);
	}
	*tlo = n;
	return n <= f;
}

static void check(const float lo[3], const float hi[3], const RtkEntriesBeam &b, const char *what)
{
	float t_full = 0.0f, t_red = 0.0f;
	const bool a_full = rtk_entries_child_full(lo, hi, b, &t_full), a_red = rtk_entries_child(lo, hi, b, &t_red);
	cases++;
	float t_control = 0.0f;
	if (control_child(lo, hi, b, &t_control) != a_full || bits(t_control) != bits(t_full)) control_bad++;
	if (a_full == a_red && bits(t_full) == bits(t_red)) return;
	if (bad++ < 10) {
		printf("MISMATCH (%s): admit %d / %d, tlo %08x / %08x\n", what, (int)a_full, (int)a_red, bits(t_full), bits(t_red));
		for (int a = 0; a < 3; a++)
			printf("  axis %d neg %u: lo %08x hi %08x olo %08x ohi %08x rlo %08x rhi %08x m %08x\n", a, (b.neg >> a) & 1u, bits(lo[a]), bits(hi[a]),
				bits(b.olo[a]), bits(b.ohi[a]), bits(b.rlo[a]), bits(b.rhi[a]), bits(b.m[a]));
		printf("  tmin %08x\n", bits(b.tmin));
	}
}

// the margin as the kernel forms it (bound = max(largest |plane| of the scene, 1))
static void margins(RtkEntriesBeam &b, float bound)
{
	for (int a = 0; a < 3; a++)
		b.m[a] = 0x1p-21f * (fmaxf(fabsf(b.rlo[a]), fabsf(b.rhi[a])) * (fmaxf(fabsf(b.olo[a]), fabsf(b.ohi[a])) + bound));
}

// a magnitude spread over many binades, denormals included now and then
static float magnitude(int emin, int emax)
{
	const int e = emin + (int)(rnd() % (uint64_t)(emax - emin + 1));
	return (1.0f + unit()) * pow2(e);
}

static float small_value()
{
	switch (rnd() % 8u) {
	case 0: return 0.0f;
	case 1: return -0.0f;
	case 2: return from_bits((uint32_t)(rnd() % 0x00800000u));                       // a positive denormal
	case 3: return -from_bits((uint32_t)(rnd() % 0x00800000u));
	case 4: return magnitude(-126, -100);
	case 5: return -magnitude(-126, -100);
	default: return (unit() - 0.5f) * 4.0f;
	}
}

static void random_beam(RtkEntriesBeam &b, bool tiny_origins)
{
	b.neg = (uint32_t)(rnd() & 7u);
	for (int a = 0; a < 3; a++) {
		float o0 = tiny_origins ? small_value() : (unit() - 0.5f) * magnitude(-10, 19), o1 = tiny_origins ? small_value() : o0 + (unit() - 0.5f) * magnitude(-20, 4);
		if (fabsf(o1) >= 0x1p19f) o1 = o0;
		if (rnd() % 4u == 0u) o1 = o0;                                                // zero-width origin box: the pinhole camera
		b.olo[a] = fminf(o0, o1); b.ohi[a] = fmaxf(o0, o1);
		float r0 = magnitude(-99, 98), r1 = rnd() % 2u ? r0 * (1.0f + unit() * 0x1p-3f) : magnitude(-99, 98);
		if (rnd() % 8u == 0u) r1 = r0;
		const float sign = ((b.neg >> a) & 1u) ? -1.0f : 1.0f;
		r0 *= sign; r1 *= sign;
		b.rlo[a] = fminf(r0, r1); b.rhi[a] = fmaxf(r0, r1);
		// the kernel's two ulps outward
		b.rlo[a] -= 0x1p-22f * fabsf(b.rlo[a]); b.rhi[a] += 0x1p-22f * fabsf(b.rhi[a]);
	}
	margins(b, 1.0f + unit() * magnitude(0, 18));
	switch (rnd() % 4u) {
	case 0: b.tmin = 0.0f; break;
	case 1: b.tmin = -magnitude(-20, 20); break;
	case 2: b.tmin = -INFINITY; break;
	default: b.tmin = magnitude(-20, 20); break;
	}
}

static float random_plane(const RtkEntriesBeam &b, int a, bool tiny)
{
	switch (rnd() % 12u) {
	case 0: return b.olo[a];                                                          // a plane equal to an origin bound
	case 1: return b.ohi[a];
	case 2: { const float p = from_bits(bits(b.olo[a]) + 1u); return p == p && fabsf(p) < INFINITY ? p : b.olo[a]; }   // ... and one step from it
	case 3: { const float p = from_bits(bits(b.ohi[a]) - 1u); return p == p && fabsf(p) < INFINITY ? p : b.ohi[a]; }
	case 4: return INFINITY;                                                          // empty slots
	case 5: return -INFINITY;
	case 6: return small_value();
	case 7: return (unit() - 0.5f) * magnitude(0, 19);
	default: return tiny ? small_value() : b.olo[a] + (unit() - 0.5f) * magnitude(-24, 6);
	}
}

static void random_case(bool tiny)
{
	RtkEntriesBeam b;
	random_beam(b, tiny);
	float lo[3], hi[3];
	for (int a = 0; a < 3; a++) {
		const float p0 = random_plane(b, a, tiny), p1 = random_plane(b, a, tiny);
		if (rnd() % 8u == 0u) { lo[a] = INFINITY; hi[a] = -INFINITY; }                // an empty slot as the builder writes it
		else if (rnd() % 16u == 0u) { lo[a] = p0; hi[a] = p1; }                         // unordered: whatever the planes are, the forms agree
		else { lo[a] = fminf(p0, p1); hi[a] = fmaxf(p0, p1); }
	}
	check(lo, hi, b, tiny ? "random, tiny origins" : "random");
}

// every combination of a few special planes, origins and reciprocals, for all eight octants
static void edge_cases()
{
	const float origins[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0x1p-149f, -0x1p-149f, 0x1p-126f, 0.5f, 0x1.fffffep18f, -0x1.fffffep18f };
	const float recips[] = { 0x1.000002p-100f, 1.0f, 0x1.8p0f, 0x1p20f, 0x1.fffffcp99f };
	const float planes[] = { 0.0f, -0.0f, 1.0f, -1.0f, 0x1p-149f, -0x1p-149f, 0x1.8p-126f, 0.5f, 0x1.000002p0f, 0x1.fffffep-1f, INFINITY, -INFINITY, 0x1p19f, -0x1p19f };
	const int no = (int)(sizeof(origins) / sizeof(origins[0])), nr = (int)(sizeof(recips) / sizeof(recips[0])), np = (int)(sizeof(planes) / sizeof(planes[0]));
	for (uint32_t neg = 0; neg < 8u; neg++)
		for (int i0 = 0; i0 < no; i0++) for (int i1 = 0; i1 < no; i1++)
			for (int r0 = 0; r0 < nr; r0++) for (int r1 = r0; r1 < nr; r1++)
				for (int p0 = 0; p0 < np; p0++) for (int p1 = 0; p1 < np; p1++) {
					RtkEntriesBeam b;
					b.neg = neg;
					float lo[3], hi[3];
					for (int a = 0; a < 3; a++) {
						// (fminf / fmaxf of a zero pair may keep either sign: both orders of -0 and +0 are among the combinations)
						b.olo[a] = origins[i0] <= origins[i1] ? origins[i0] : origins[i1];
						b.ohi[a] = origins[i0] <= origins[i1] ? origins[i1] : origins[i0];
						const float s = ((neg >> a) & 1u) ? -1.0f : 1.0f;
						b.rlo[a] = s > 0.0f ? recips[r0] : -recips[r1];
						b.rhi[a] = s > 0.0f ? recips[r1] : -recips[r0];
						// axis 0 as given, axis 1 with the planes swapped, axis 2 a box that always passes
						lo[a] = a == 0 ? planes[p0] : a == 1 ? planes[p1] : -INFINITY;
						hi[a] = a == 0 ? planes[p1] : a == 1 ? planes[p0] : INFINITY;
					}
					margins(b, 1.0f);
					b.tmin = (p0 & 1) ? 0.0f : -0x1p-3f;
					check(lo, hi, b, "edge");
				}
}

int main(int argc, char **argv)
{
	const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000ull;
	rng_state = (argc > 2 ? strtoull(argv[2], nullptr, 10) : 1ull) * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull;
	edge_cases();
	const unsigned long long edges = cases;
	for (unsigned long long i = 0; i < n; i++) random_case((i & 3ull) == 3ull);
	if (bad) { printf("%llu of %llu cases differ\n", bad, cases); return 1; }
	printf("ok %llu edge %llu random %llu control\n", edges, cases - edges, control_bad);
	return 0;
}
