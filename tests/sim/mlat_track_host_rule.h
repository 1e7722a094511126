// mlat_track_host_rule.h -- TEST INFRASTRUCTURE ONLY.  What the two drivers of the MLAT track store's kernels --
// tests/sim/mlat_track_driver.cpp (the SIMT emulator, on the CPU) and tests/gpu/mlat_track_device_driver.hip (the shipped
// translation unit, on the GPU) -- restate of the host's rule in adsb_hip.hip, stated once for both: the track rule's argument
// table, the work buffer carved by adsb_mlat_track.h's layout() before the first launch with guard bytes between and behind its
// parts, the counts read between the launchers with their range checks (the host's -EIO, the drivers' -5), the other buffer
// given room for nt + nk rows before the launch that needs it, -ENOSPC decided before the gather with nothing written.  The
// drivers give the memory: a Part (make / back / p / host, as tests/gpu/device_buffers.h's) and end(launched, parts), which
// drains the launches and brings every part back whole.  Host code only; needs adsb_mlat_track.h.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <string.h>

#include <initializer_list>
#include <utility>
#include <vector>

namespace track_rule {
namespace th = adsb_mlat_track_host;

constexpr unsigned char kGuardByte = 0xA5;

// adsb_mlat_track_rule as the drivers are given it
struct Rule {
  double alpha, beta, gate_m, max_speed_mps, max_gap_s, max_rms_m, min_up_m;
  int restart_after, reserved;
};
static_assert(sizeof(Rule) == th::kRuleBytes, "adsb_mlat_track_rule");

inline bool finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }
// adsb_stream_mlat_track's -EINVAL for the track rule
inline bool rule_refused(const void* rule) {
  if (!rule) return true;
  Rule r;
  memcpy(&r, rule, sizeof r);
  if (!(finite(r.alpha) && r.alpha > 0.0 && r.alpha <= 1.0) || !(finite(r.beta) && r.beta > 0.0 && r.beta <= 1.0)) return true;
  if (!(finite(r.gate_m) && r.gate_m >= 0.0) || !(finite(r.max_speed_mps) && r.max_speed_mps >= 0.0) || !(finite(r.max_gap_s) && r.max_gap_s >= 0.0))
    return true;
  return r.max_rms_m != r.max_rms_m || r.min_up_m != r.min_up_m || r.restart_after < 1 || r.reserved != 0;
}

// (offset, bytes in use) of every part of layout(n), in carve()'s order
inline std::vector<std::pair<size_t, size_t>> parts(const th::Layout& L, size_t n) {
  const size_t chunks = (n + th::kChunk - 1) / th::kChunk + 1;
  return {{L.cnts, th::kCntWords * 4}, {L.stats, th::kStatWords * 8}, {L.w, n * 4}, {L.cnt, chunks * 4}, {L.sel, n * 4}, {L.run_start, n * 4},
          {L.run_len, n * 4}, {L.pos, n * 4}, {L.newidx, n * 4}, {L.keys, n * 8}, {L.keys_tmp, n * 8}, {L.vals, n * 4}, {L.vals_tmp, n * 4},
          {L.hist, adsb_shared_host::sort_hist_bytes((int)n)}};
}
// every byte between a part's end and the next part's start (or the tail's end) is still the guard's
inline bool guards_ok(const unsigned char* raw, size_t raw_bytes, const std::vector<std::pair<size_t, size_t>>& p) {
  for (size_t k = 0; k < p.size(); ++k) {
    const size_t end = k + 1 < p.size() ? p[k + 1].first : raw_bytes;
    if (p[k].first + p[k].second > end) return false;
    for (size_t q = p[k].first + p[k].second; q < end; ++q) if (raw[q] != kGuardByte) return false;
  }
  return true;
}

// One adsb_stream_mlat_track call behind the solve: fixes[ng] (and aux[ng], may be null) -> store_out (room for nt + ng rows:
// the store after the call, *nt_out rows; a refused call or one without eligible fixes copies the store), stats[8] in
// adsb_mlat_track_stats' order.  0; -22 (arguments); -1: a guard byte or a read-only part was written; -5: a count out of
// range; or the sticky HIP code.
template <class Part, class End>
int update(End end, const void* fixes, const void* aux, int ng, const void* rule, const void* store, int nt, void* store_out, int* nt_out,
           long long* stats) {
  if (rule_refused(rule) || ng < 0 || nt < 0) return -22;
  for (int k = 0; k < 8; ++k) stats[k] = 0;
  stats[0] = ng; stats[7] = nt;
  *nt_out = nt;
  if (nt) memcpy(store_out, store, (size_t)nt * th::kRowBytes);
  if (ng == 0) return 0;
  const th::Layout L = th::layout((size_t)ng);
  const auto P = parts(L, (size_t)ng);
  Part p_fix, p_aux, p_store, p_work, p_next;
  int rc;
  if ((rc = p_fix.make(fixes, (size_t)ng * th::kFixBytes, true)) || (rc = p_aux.make(aux, aux ? (size_t)ng * th::kAuxBytes : 0, true)) ||
      (rc = p_store.make(nt ? store : nullptr, (size_t)nt * th::kRowBytes, true)) || (rc = p_work.make(nullptr, L.bytes, false)))
    return rc;
  if ((rc = end(th::launch_keys(nullptr, p_fix.p, ng, p_work.p, L), {&p_fix, &p_work}))) return rc;
  if (!guards_ok(p_work.host.data(), p_work.host.size(), P)) return -1;
  const int nk = ((const int*)(p_work.host.data() + L.cnts))[th::kCntKeys];
  if (nk < 0 || nk > ng) return -5;
  stats[1] = nk;
  if (nk == 0) return 0;
  if ((rc = p_next.make(nullptr, ((size_t)nt + (size_t)nk) * th::kRowBytes, false))) return rc;
  if ((rc = end(th::launch_update(nullptr, p_fix.p, aux ? p_aux.p : nullptr, nk, rule, p_store.p, nt, p_next.p, p_work.p, L),
                {&p_fix, &p_aux, &p_store, &p_work, &p_next})))
    return rc;
  if (!guards_ok(p_work.host.data(), p_work.host.size(), P)) return -1;
  const int* const cnts = (const int*)(p_work.host.data() + L.cnts);
  const int nr = cnts[th::kCntRuns], nn = cnts[th::kCntNew];
  if (nr < 1 || nr > nk || nn < 0 || nn > nr) return -5;
  const size_t used = ((size_t)nt + (size_t)nn) * th::kRowBytes;
  for (size_t q = used; q < p_next.bytes; ++q) if (p_next.host[q] != kGuardByte) return -1;      // no row behind the store's new end
  memcpy(store_out, p_next.host.data(), used);
  *nt_out = nt + nn;
  const unsigned long long* const s = (const unsigned long long*)(p_work.host.data() + L.stats);
  stats[2] = (long long)s[th::kStatUnusable]; stats[3] = (long long)s[th::kStatStale]; stats[4] = (long long)s[th::kStatRejected];
  stats[5] = (long long)s[th::kStatTaken]; stats[6] = (long long)s[th::kStatStarted]; stats[7] = nt + nn;
  return 0;
}

// adsb_stream_mlat_tracks (expire false: rows[cap]; -28 with *n stated and nothing written) and adsb_stream_mlat_tracks_expire
// (expire true: the kept rows into rows[nt], *n of them; min_fixes is not read)
template <class Part, class End>
int read(End end, const void* store, int nt, int min_fixes, double cutoff, bool expire, void* rows, int cap, int* n) {
  if (nt < 0 || cutoff != cutoff || !n || (!expire && (cap < 0 || (cap > 0 && !rows)))) return -22;
  *n = 0;
  if (nt == 0) return 0;
  const th::Layout L = th::layout((size_t)nt);
  const auto P = parts(L, (size_t)nt);
  Part p_store, p_work, p_out;
  int rc;
  if ((rc = p_store.make(store, (size_t)nt * th::kRowBytes, true)) || (rc = p_work.make(nullptr, L.bytes, false))) return rc;
  if ((rc = end(th::launch_pick(nullptr, p_store.p, nt, expire ? INT_MIN : min_fixes, cutoff, p_work.p, L), {&p_store, &p_work}))) return rc;
  if (!guards_ok(p_work.host.data(), p_work.host.size(), P)) return -1;
  const int k = ((const int*)(p_work.host.data() + L.cnts))[th::kCntKeys];
  if (k < 0 || k > nt) return -5;
  *n = k;
  if (!expire && k > cap) return -28;
  if (k == 0) return 0;
  if ((rc = p_out.make(nullptr, (size_t)k * th::kRowBytes, false))) return rc;
  if ((rc = end(th::launch_gather(nullptr, p_store.p, k, p_out.p, p_work.p, L), {&p_store, &p_work, &p_out}))) return rc;
  if (!guards_ok(p_work.host.data(), p_work.host.size(), P)) return -1;
  memcpy(rows, p_out.host.data(), (size_t)k * th::kRowBytes);
  return 0;
}

}  // namespace track_rule
