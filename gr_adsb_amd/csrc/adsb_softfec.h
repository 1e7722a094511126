// adsb_softfec.h -- the launchers of adsb_softfec.hip (ADSB_FLAG_FEC_SOFT's kernels: adsb_softfec_device.h), for adsb_hip.hip.
// Plain pointers only, as adsb_mlat.h: the translation units share no type.  Every call queues one kernel on `stream` (a
// hipStream_t) and returns the hipError_t of the launch as an int (0: queued).  Internal to libadsb_hip.so.
#pragma once

namespace adsb_softfec_host {

constexpr int kRowBytes = 8, kRuleBytes = 16, kRecWords = 4, kWavesPerGroup = 4;

// The delivered records of one pass, in place, behind k_fec: out[*n_kept] (at most out_cap) records of four words, the pinned
// mirror of the first host_cap of them (null: none), rows[out_cap].  mode: ADSB_FMT_*; data / n / origin / scale / sps: the
// pass's samples as k_confidence reads them.  rule: kRuleBytes of adsb_soft_fec_rule, in host memory.
int launch_records(void* stream, unsigned grid, int mode, const void* data, long long n, long long origin, float scale, int sps,
                   const void* rule, void* out, const int* n_kept, int out_cap, void* host_out, int host_cap, void* rows);
// The slices of adsb_demod_work, behind k_fec_slices: bits14 / ok / tag_idx of ntags tags over the float chunk data[n]; rows[ntags]
int launch_slices(void* stream, unsigned grid, const void* data, long long n, const long long* tag_idx, int sps, const void* rule,
                  unsigned char* bits14, unsigned char* ok, int ntags, void* rows);

}  // namespace adsb_softfec_host
