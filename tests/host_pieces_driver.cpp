// Driver of tests/test_host_pieces_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_host_pieces.h alone (no HIP), with the
// address and undefined-behaviour sanitizers. Every buffer is allocated at exactly the size the header states and written or read
// in full, so a piece that leaves its allocation is an error of the run. Every line of standard input is one command, answered
// by one line:
//   consts                 ZERO_COPY_RAYS PIPE_CHUNK_RAYS CAND_SLOTS CAND_RAYS
//   staging N              capacity bytes, then the offsets of rays records after hits mask status (every piece is filled)
//   cand                   bytes, then the offsets of the records, the full hits, the counts (every piece is filled)
//   band W H | candk R | ticket T      the one number
//   pipe N CHUNK E F       run_pipeline with recording callables; enqueue call number E / finish call number F fails (-1: none);
//                          finish answers with the piece's size. The result (-1: failed), then the calls: eSLOT:AT:M fSLOT:AT:M ...
//   rounds N K S           run_candidate_rounds over a synthetic scene: ray i, with s = i + S, has (0, 1, K - 1, K, K + 1, 100, 150)[s % 7]
//                          candidates, candidate j at t = j + 1 with primitive j, and rejects the first (5 s + s / 7) % 160 of them.
//                          The result, the rounds, the wrongs (an offer out of order or twice, a ray that went on after a list
//                          short of k, a hit that is not the ray's), then per ray ACCEPTED:OFFERS (-1: a miss)
//   leak                   16 bytes nobody frees: the run must not end clean
#include "rtk_host_pieces.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>

static std::string g_error;
void rtk_set_error(const char *fmt, ...)
{
	char text[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(text, sizeof(text), fmt, ap);
	va_end(ap);
	g_error = text;
}

static void staging(size_t n)
{
	const size_t cap = staging_capacity(n), bytes = Staging::bytes(cap);
	char *base = static_cast<char *>(malloc(bytes));
	const Staging s(base, cap);
	memset(s.rays, 1, cap * sizeof(rtk_ray));
	memset(s.rec, 2, cap * sizeof(rtk_hit_record));
	memset(s.after, 3, cap * sizeof(rtk_hit_record));
	memset(s.hits, 4, cap * sizeof(rtk_hit));
	memset(s.mask, 5, cap * 4);
	memset(s.status, 6, 64);
	std::cout << cap << ' ' << bytes << ' ' << (char *)s.rays - base << ' ' << (char *)s.rec - base << ' ' << (char *)s.after - base << ' '
		<< (char *)s.hits - base << ' ' << (char *)s.mask - base << ' ' << (char *)s.status - base << "\n";
	free(base);
}

static void candidates()
{
	char *base = static_cast<char *>(malloc(CandStaging::bytes()));
	const CandStaging s(base);
	memset(s.cand, 1, CAND_SLOTS * sizeof(rtk_hit_record));
	memset(s.hits, 2, CAND_SLOTS * sizeof(rtk_hit));
	memset(s.count, 3, CAND_RAYS * sizeof(uint32_t));
	std::cout << CandStaging::bytes() << ' ' << (char *)s.cand - base << ' ' << (char *)s.hits - base << ' ' << (char *)s.count - base << "\n";
	free(base);
}

static void pipe(size_t n, size_t chunk, long fail_enqueue, long fail_finish)
{
	std::ostringstream calls;
	long enqueues = 0, finishes = 0;
	const size_t r = run_pipeline(n, chunk,
		[&](int slot, size_t at, size_t m) { calls << " e" << slot << ':' << at << ':' << m; return enqueues++ != fail_enqueue; },
		[&](int slot, size_t at, size_t m) { calls << " f" << slot << ':' << at << ':' << m; return finishes++ != fail_finish ? m : (size_t)-1; });
	std::cout << (long long)r << calls.str() << "\n";
}

static void rounds(size_t n, size_t first_k, size_t shift)
{
	const size_t lengths[7] = { 0, 1, first_k - 1, first_k, first_k + 1, 100, 150 };
	auto length = [&](size_t i) { return lengths[(i + shift) % 7]; };
	auto rejects = [&](size_t i) { return (5 * (i + shift) + (i + shift) / 7) % 160; };
	std::vector<rtk_hit> hits(n);
	std::vector<uint8_t> mask(n, 0xaa);
	std::vector<uint32_t> offers(n, 0), last_have(n, 0), last_k(n, 0);
	std::vector<rtk_hit_record> cand;
	std::vector<rtk_hit> cand_hits;
	std::vector<uint32_t> count;
	long num_rounds = 0, wrongs = 0;
	auto round = [&](const std::vector<size_t> &todo, const std::vector<rtk_hit_record> &after, size_t k) {
		num_rounds++;
		const size_t r = todo.size();
		if (after.size() != r || k != cand_k(r)) wrongs++;
		cand = std::vector<rtk_hit_record>(r * k, rtk_hit_record{ 0.0f, 0.0f, 0.0f, RTK_PRIM_NONE });      // (exactly r * k: a read past a list's end is caught)
		cand_hits = std::vector<rtk_hit>(r * k);
		count = std::vector<uint32_t>(r);
		for (size_t q = 0; q < r; q++) {
			const size_t i = todo[q];
			size_t first = 0;
			if (after[q].prim != RTK_PRIM_NONE) {
				first = (size_t)after[q].prim + 1;
				if (after[q].t != (float)first || last_have[i] != last_k[i] || first != offers[i]) wrongs++;      // (a short list, or not the last one offered)
			} else if (offers[i] != 0) wrongs++;
			const size_t left = length(i) > first ? length(i) - first : 0;
			count[q] = (uint32_t)(left < k ? left : k);
			last_have[i] = count[q]; last_k[i] = (uint32_t)k;
			for (size_t j = 0; j < count[q]; j++) {
				cand[q * k + j] = rtk_hit_record{ (float)(first + j + 1), 0.0f, 0.0f, (uint32_t)(first + j) };
				rtk_hit &h = cand_hits[q * k + j];
				memset(&h, 0, sizeof(h));
				h.t = (float)(first + j + 1); h.mesh_index = (uint32_t)i; h.triangle_index = (uint32_t)(first + j);
			}
		}
		return CandRound{ cand.data(), cand_hits.data(), count.data() };
	};
	const size_t result = run_candidate_rounds(n, hits.data(), mask.data(), round, [&](size_t i, const rtk_hit *hit) {
		if (hit->mesh_index != i || hit->triangle_index != offers[i]) wrongs++;      // every candidate in order, exactly once
		offers[i]++;
		return hit->triangle_index >= rejects(i);
	});
	std::cout << (long long)result << ' ' << num_rounds << ' ' << wrongs;
	for (size_t i = 0; i < n; i++) {
		if (mask[i] > 1 || (mask[i] && hits[i].mesh_index != i)) { std::cout << " bad"; continue; }
		std::cout << ' ' << (mask[i] ? (long)hits[i].triangle_index : -1L) << ':' << offers[i];
	}
	std::cout << "\n";
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		long long a = 0, b = 0, c = -1, d = -1;
		in >> cmd >> a >> b >> c >> d;
		if (cmd == "consts") std::cout << ZERO_COPY_RAYS << ' ' << PIPE_CHUNK_RAYS << ' ' << CAND_SLOTS << ' ' << CAND_RAYS << "\n";
		else if (cmd == "staging") staging((size_t)a);
		else if (cmd == "cand") candidates();
		else if (cmd == "band") std::cout << band_rays((uint32_t)a, (uint32_t)b) << "\n";
		else if (cmd == "candk") std::cout << cand_k((size_t)a) << "\n";
		else if (cmd == "ticket") std::cout << next_ticket((uint32_t)a) << "\n";
		else if (cmd == "pipe") pipe((size_t)a, (size_t)b, (long)c, (long)d);
		else if (cmd == "rounds") rounds((size_t)a, (size_t)b, (size_t)(c < 0 ? 0 : c));
		else if (cmd == "leak") { void *volatile p = malloc(16); p = nullptr; (void)p; }
		else { std::cerr << "bad command: " << line << "\n"; return 2; }
		if (!g_error.empty()) { std::cerr << "unexpected error: " << g_error << "\n"; return 3; }
	}
	return 0;
}
