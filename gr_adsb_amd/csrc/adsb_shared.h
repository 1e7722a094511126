// adsb_shared.h -- the launchers of adsb_shared.hip (ADSB_FLAG_STREAM_DECODE_SHARED: adsb_shared_device.h), for adsb_hip.hip.
// Plain pointers only: the two translation units share no type.  Every call queues its kernels on `stream` (a hipStream_t)
// and returns the hipError_t of the launches as an int (0: queued).  Internal to libadsb_hip.so: not part of the C ABI.
#pragma once
#include <stddef.h>

namespace adsb_shared_host {

constexpr int kRecBytes = 32, kRowBytes = 72;      // what the unit moves as opaque words (adsb_hip.hip: static_asserts)
constexpr int kSortTile = 4096;
// bytes of the histogram the sort needs for n pairs
size_t sort_hist_bytes(int n);
// recs[n] (32 bytes each, offset in word 0), first[n_items + 1], start[n_items] -> keys[n], vals[n] = 0 .. n-1, ts[n]
int launch_keys(void* stream, const void* recs, int n, const int* first, const double* start, int n_items, double fs,
                unsigned long long* keys, unsigned* vals, double* ts);
// A stable sort of the pairs by key.  keys / vals hold the result; keys_tmp / vals_tmp [n] and hist are scratch.
int launch_sort(void* stream, unsigned long long* keys, unsigned* vals, unsigned long long* keys_tmp, unsigned* vals_tmp, int n,
                unsigned* hist);
// sorted_recs[r] = recs[vals[r]], sorted_ts[r] = ts[vals[r]], order[r] = vals[r]
int launch_gather(void* stream, const void* recs, const double* ts, const unsigned* vals, int n, void* sorted_recs, double* sorted_ts,
                  int* order);
// recs[order[r]].word 3 = sorted_recs[r].word 3, rows[order[r]] = sorted_rows[r] (72 bytes each)
int launch_scatter(void* stream, const void* sorted_recs, const void* sorted_rows, const int* order, int n, void* recs, void* rows);

}  // namespace adsb_shared_host
