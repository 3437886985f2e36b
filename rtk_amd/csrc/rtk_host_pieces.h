// rtk_host_pieces.h -- internal, host only (no HIP): how the host-pointer calls (rtk_trace_rays, rtk_trace_rays_filter:
// rtk_host_calls.hip) cut a batch into pieces -- the sizes, the layout of a staging allocation, the bands of an image, the
// order of a two-slot pipeline, the rounds of a host-callback filter. What a piece or a round does on the GPU is the
// caller's, handed in as a callable (recording ones in tests/host_pieces_driver.cpp).
#pragma once

#include "rtk_amd.h"

#include <string.h>

#include <vector>

void rtk_set_error(const char *fmt, ...);

const size_t ZERO_COPY_RAYS = 2048;              // pieces up to this size are read and written in place by the kernels
const size_t PIPE_CHUNK_RAYS = (size_t)1 << 15;  // rays per piece when a batch is pipelined (batches of two pieces and more are)
const size_t CAND_SLOTS = (size_t)1 << 16;       // candidate records per round (4.4 MB of full hits)
const size_t CAND_RAYS = (size_t)1 << 14;        // rays per round of a host-callback filter call: at least 4 candidates each

// rays a staging allocation is made for when `n` are asked for
inline size_t staging_capacity(size_t n) { size_t want = 64; while (want < n) want <<= 1; return want; }

// One staging allocation for `cap` rays, pinned or on the device: [rays | records | after | hits | mask | status], each
// beginning where the one before it ends
struct Staging {
	rtk_ray *rays = nullptr;
	rtk_hit_record *rec = nullptr, *after = nullptr;
	rtk_hit *hits = nullptr;
	uint8_t *mask = nullptr;                   // (4 bytes per ray: what follows stays aligned)
	unsigned long long *status = nullptr;      // 64 bytes; the pinned one receives the launch-error word and the ticket
	static size_t bytes(size_t cap) { return cap * (sizeof(rtk_ray) + 2 * sizeof(rtk_hit_record) + sizeof(rtk_hit) + 4) + 64; }
	Staging() = default;
	Staging(char *base, size_t cap)
		: rays((rtk_ray *)base), rec((rtk_hit_record *)(rays + cap)), after(rec + cap), hits((rtk_hit *)(after + cap)),
		  mask((uint8_t *)(hits + cap)), status((unsigned long long *)(mask + 4 * cap)) {}
};

// The candidate lists of a host-callback filter, one allocation as well: CAND_SLOTS records and their full hits, k = cand_k(rays)
// of them per ray, and how many of each ray's are valid
struct CandStaging {
	rtk_hit_record *cand = nullptr;
	rtk_hit *hits = nullptr;
	uint32_t *count = nullptr;
	static size_t bytes() { return CAND_SLOTS * (sizeof(rtk_hit_record) + sizeof(rtk_hit)) + CAND_RAYS * sizeof(uint32_t); }
	CandStaging() = default;
	explicit CandStaging(char *base) : cand((rtk_hit_record *)base), hits((rtk_hit *)(cand + CAND_SLOTS)), count((uint32_t *)(hits + CAND_SLOTS)) {}
};
inline size_t cand_k(size_t rays_in_round) { return CAND_SLOTS / rays_in_round < 64 ? CAND_SLOTS / rays_in_round : 64; }

// pieces of one workgroup are waited for by their ticket: 0 means "none"
inline uint32_t next_ticket(uint32_t ticket) { return ticket == 0xffffffffu ? 1u : ticket + 1u; }

// A pipelined batch that is a row-major iw x ih image goes in bands of whole 64-pixel rows, each announced to its launch as the
// image it is: rays per band (the last one may be lower), 0 = no bands. Rows double while a band stays within 2^18 rays.
inline size_t band_rays(uint32_t iw, uint32_t ih)
{
	if (iw < 128u || (iw % 64u) != 0u || (ih % 64u) != 0u || (size_t)iw * 64u > ((size_t)1 << 21)) return 0;
	size_t band_rows = 64;
	while ((band_rows * 2) * (size_t)iw <= ((size_t)1 << 18) && band_rows * 2 <= ih) band_rows *= 2;
	return band_rows * (size_t)iw;
}

// Two staging sets on two streams: while the GPU works on one piece the host copies the previous piece's results out
// and the next piece's rays in. enqueue(slot, at, m) -> bool puts rays [at, at + m) on their way in slot 0 / 1;
// finish(slot, at, m) -> hits of that piece, (size_t)-1 on error, waits for it and hands its results out. A slot's older piece
// is finished before the slot is used again, nothing is enqueued after the first failure, and what is still in flight then is
// drained in submission order. Returns the hits, (size_t)-1 if anything failed.
template <class Enqueue, class Finish>
size_t run_pipeline(size_t n, size_t chunk, Enqueue enqueue, Finish finish)
{
	size_t count = 0, piece = 0;
	size_t at_of[2] = { 0, 0 }, n_of[2] = { 0, 0 };
	bool busy[2] = { false, false }, failed = false;
	auto finish_slot = [&](int k) {
		if (!busy[k]) return;
		busy[k] = false;
		const size_t r = finish(k, at_of[k], n_of[k]);
		if (r == (size_t)-1) failed = true; else count += r;
	};
	for (size_t at = 0; at < n; at += chunk, piece++) {
		const int k = (int)(piece & 1u);
		finish_slot(k);
		const size_t m = n - at < chunk ? n - at : chunk;
		if (failed || !enqueue(k, at, m)) { failed = true; break; }
		busy[k] = true; at_of[k] = at; n_of[k] = m;
	}
	for (int j = 0; j < 2; j++) finish_slot((int)((piece + (size_t)j) & 1u));      // (the older piece first)
	return failed ? (size_t)-1 : count;
}

// What one round of a host-callback filter call brings home: lists of k records (and their full hits) per ray of the round, in
// increasing (t, primitive id) order, and how many of each list are valid. cand == NULL: the round failed.
struct CandRound { const rtk_hit_record *cand; const rtk_hit *hits; const uint32_t *count; };

// The rounds of rtk_trace_rays_filter: CAND_RAYS rays at a time; round(todo, after, k) -> CandRound collects the k closest
// candidates after `after[q]` of every undecided ray todo[q]; accept(i, hit) -> bool is asked about them in order. A ray whose
// k candidates were all rejected goes into the next round, restricted to what comes after the last one. Returns the accepted
// hits, (size_t)-1 on error.
template <class Round, class Accept>
size_t run_candidate_rounds(size_t n, rtk_hit *hits, uint8_t *hit_mask, Round round, Accept accept)
{
	size_t count = 0;
	std::vector<size_t> todo, next;
	std::vector<rtk_hit_record> after, next_after;
	for (size_t at = 0; at < n; at += CAND_RAYS) {
		const size_t m = n - at < CAND_RAYS ? n - at : CAND_RAYS;
		todo.resize(m);
		for (size_t i = 0; i < m; i++) todo[i] = at + i;
		after.assign(m, rtk_hit_record{ 0.0f, 0.0f, 0.0f, RTK_PRIM_NONE });
		if (hit_mask) memset(hit_mask + at, 0, m);
		for (unsigned rounds = 0; !todo.empty(); rounds++) {
			if (rounds > (1u << 16)) { rtk_set_error("rtk_trace_rays_filter: a ray had more than 2^18 rejected candidates"); return (size_t)-1; }
			const size_t r = todo.size(), k = cand_k(r);
			const CandRound got = round(todo, after, k);
			if (!got.cand) return (size_t)-1;
			next.clear();
			next_after.clear();
			for (size_t q = 0; q < r; q++) {
				const size_t i = todo[q];
				const uint32_t have = got.count[q];
				bool accepted = false;
				for (uint32_t j = 0; j < have && !accepted; j++) {
					if (accept(i, &got.hits[q * k + j])) {
						accepted = true;
						count++;
						if (hits) hits[i] = got.hits[q * k + j];
						if (hit_mask) hit_mask[i] = 1;
					}
				}
				if (!accepted && have == k) {                                      // the list was full: there may be more behind it
					next.push_back(i);
					next_after.push_back(got.cand[q * k + k - 1]);
				}
			}
			todo.swap(next);
			after.swap(next_after);
		}
	}
	return count;
}
