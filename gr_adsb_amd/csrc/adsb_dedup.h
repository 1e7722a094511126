// adsb_dedup.h -- the launchers of adsb_dedup.hip (ADSB_FLAG_STREAM_DEDUP: adsb_dedup_device.h), for adsb_hip.hip.
// Plain pointers only, as adsb_shared.h: the translation units share no type.  Every call queues its kernels on `stream` (a
// hipStream_t) and returns the hipError_t of the launches as an int (0: queued).  Internal to libadsb_hip.so.
#pragma once
#include <stddef.h>

namespace adsb_dedup_host {

constexpr int kRecBytes = 32, kRowBytes = 72, kEntBytes = 32;
// what k_dedup_merge leaves behind: the next carry is out[off .. off + cnt), hi its last timestamp
struct State { int off, cnt; double hi; };

// sorted_recs / sorted_ts / order [n]: k_shared_gather's output; first[n_items + 1], item_stream[n_items] -> ent[n]
int launch_entries(void* stream, const void* sorted_recs, const double* sorted_ts, const int* order, int n, const int* first,
                   const int* item_stream, int n_items, void* ent);
// ent[n] against itself and carry[nc] -> dup[n] at list positions; duplicates lose ADSB_BURST_DEMOD in sorted_recs
int launch_find(void* stream, const void* ent, int n, const void* carry, int nc, double window, const int* order, void* sorted_recs,
                int* dup);
// out[nc + n] = carry and ent merged; *state (device memory): the cut at hi - horizon
int launch_merge(void* stream, const void* carry, int nc, const void* ent, int n, double horizon, void* out, void* state);
// the delivered records and rows of the duplicates: ADSB_BURST_DEMOD back, port = ADSB_DEC_DUPLICATE
int launch_mark(void* stream, const int* dup, int n, void* recs, void* rows);

}  // namespace adsb_dedup_host
