// adsb_plan.h -- host-side index bookkeeping shared by libadsb_hip.so and the test emulator driver:
// how one reference work() call (or one overlapped shard) maps onto k_detect's local index space, and
// how the framer's two words of cross-call state evolve.  Pure C++, no HIP, no arithmetic on samples.
//
// Local index i of the device buffer <-> framer in0 index j = i - in0_base <-> stream offset origin + i.
// Citations: /root/reference/python/adsb/framer.py, demod.py.
#pragma once

#include "../../include/adsb_hip.h"      // the record flag bits

namespace adsb {

// Samples the re-trigger gate stays closed behind a record: 63 symbols (framer.py:165), 119 behind a record that a
// long-aware context flagged ADSB_BURST_LONG_HINT.  THE statement of the window for every host-side gate.
inline long long gate_window(unsigned flags, int sps) { return ((flags & ADSB_BURST_LONG_HINT) ? 119ll : 63ll) * sps; }

struct Plan {
  int mode;                 // 0 complex64 IQ, 1 float |IQ|^2
  const void* d_data;
  long long n;              // samples in the buffer
  long long in0_base;       // local index of in0[0]
  long long scan_lo, scan_hi;   // thresholded range == in0[0:N] (framer.py:83-84)
  long long fall_hi;        // falls must lie below (framer.py:102-108 drops a pulse still high at N)
  long long dem_hi;         // end of the demod input (demod.py:82)
  long long origin;         // stream offset of local index 0
  float prev_in0;           // framer.py:54,84,87
  int end_is_call_end;
  long long prev_eob_stream;    // framer.py:57 expressed as a stream offset
  bool gate;                // apply framer.py:121-123 on the device
  int head_n = 0;           // shard mode: deliver the first head_n centres whether gated or not
  bool long_aware = false;  // opt-in length-aware gate (never in GNU Radio emulation): set by the caller from the context
  bool air = false;         // ADSB_FLAG_AIRCRAFT_TABLE: the pass is published, its records get the table step (canonical calls)
};

// How a pass over `ntiles` tiles (1024 samples each) is cut into chunks, one per wavefront, for a device that keeps
// `resident` wavefronts of k_detect resident at a time.  One resident round is the floor (units == ntiles while there
// are fewer tiles than resident wavefronts); a bulk pass is cut into up to kChunkRounds rounds of shorter chunks, none
// shorter than kMinChunkTiles tiles: the wavefronts of ONE round, each with 1/resident of the stream, finish up to 10 %
// apart (their burst counts differ) and the kernel ends with its slowest wavefront; with several rounds the dispatcher
// evens that out.  Measured on MI355X (tools/r3_variants.sh): 2^30 complex64 samples 0.74 -> 0.79-0.82 of the HBM peak
// with 8 rounds (16: the same for complex64, -6 % for int8 / int16; 4: -3 %), 2^28 samples 0.72 -> 0.79 with chunks
// down to 4 tiles (8: 0.77), 2^26 samples +1 %.
// Out: *units wavefronts with work, each *tiles_per tiles long (the last may be shorter): units * tiles_per >= ntiles.
constexpr int kChunkRounds = 8, kMinChunkTiles = 4;
inline void plan_chunks(long long ntiles, long long resident, long long* units_out, long long* tiles_per_out) {
  if (ntiles < 1) ntiles = 1;
  if (resident < 1) resident = 1;
  long long rounds = ntiles / (resident * kMinChunkTiles);
  if (rounds < 1) rounds = 1;
  if (rounds > kChunkRounds) rounds = kChunkRounds;
  const long long umax = resident * rounds;
  long long units = ntiles < umax ? ntiles : umax;
  const long long tiles_per = (ntiles + units - 1) / units;
  units = (ntiles + tiles_per - 1) / tiles_per;
  *units_out = units;
  *tiles_per_out = tiles_per;
}

struct FramerState {
  float prev_in0 = 0.0f;    // framer.py:54
  long long prev_eob = -1;  // framer.py:57 (index into the NEXT call's in0)
};

// One canonical whole-buffer call on a fresh stream: history = 8*sps-1 zeros, N = n, then demod over
// the same n samples (SURVEY.md §8a "chunk semantics").
inline Plan plan_canonical(int mode, const void* d, long long n, long long abs_offset, int sps) {
  const long long H = 8ll * sps;
  Plan p;
  p.mode = mode; p.d_data = d; p.n = n;
  p.in0_base = -(H - 1); p.scan_lo = p.in0_base; p.scan_hi = n - (H - 1); p.fall_hi = p.scan_hi;
  p.dem_hi = n; p.origin = abs_offset; p.prev_in0 = 0.0f; p.end_is_call_end = 1;
  p.prev_eob_stream = abs_offset + p.in0_base - 1;      // prev_eob_idx = -1
  p.gate = true;
  return p;
}

// One item of a batch (adsb_process_batch*: k_batch, one four-wavefront workgroup per item): the item is a canonical call cut
// into four chunks of whole tiles, as the one-launch small pass cuts its input, with the ordinary pass's first list capacity
// (chunk/256 + 64 slots per list, never more than there can be rises; whole 128-byte lines).  An item whose lists overflow is
// run again through the ordinary pass by the host, which regrows its capacity itself.
constexpr long long kBatchItemMax = 1ll << 22;      // ADSB_BATCH_ITEM_MAX
struct BatchGeom { long long ntiles, chunk; int rec_cap, long_cap; };
inline BatchGeom plan_batch_item(long long n, int sps, int lists = 4, int tile = 1024) {
  const long long span = n - (8ll * sps - 1);             // plan_canonical: scan_hi
  long long ntiles = span > 0 ? (span + tile - 1) / tile : 0;
  if (ntiles < 1) ntiles = 1;
  const long long tiles_per = (ntiles + lists - 1) / lists;
  BatchGeom g;
  g.ntiles = ntiles; g.chunk = tiles_per * tile;
  long long rc = g.chunk / 256 + 64;
  if (rc > g.chunk / 2 + 8) rc = g.chunk / 2 + 8;
  g.rec_cap = (int)((rc + 15) & ~15ll);
  g.long_cap = (int)(ntiles + 1);                         // at most one long pulse per tile, plus the virtual rise
  return g;
}

// Scratch of ONE batch item inside one buffer, as byte offsets from `base` (every array on a 128-byte line): the four lists'
// words and records, the ordered list and its sources, the item's gated records, the segment counts, the long-pulse list.
// Per list slot that is 8 + 32 + 8 + 4 + 32 = 84 bytes: ~0.33 bytes per sample plus ~22 KB per item.
struct BatchLay { size_t cands, sorted, recs, out, src, seg, lng, end; long long slots; BatchGeom g; };
inline BatchLay plan_batch_layout(size_t base, const BatchGeom& g, int lists, int threads, size_t rec_bytes, size_t long_bytes) {
  auto up = [](size_t v) { return (v + 127) & ~(size_t)127; };
  BatchLay L;
  L.g = g; L.slots = (long long)lists * g.rec_cap;
  const size_t s = (size_t)L.slots;
  size_t o = base;
  L.cands = o; o += up(s * 8);
  L.sorted = o; o += up(s * 8);
  L.recs = o; o += up(s * rec_bytes);
  L.out = o; o += up(s * rec_bytes);
  L.src = o; o += up(s * 4);
  L.seg = o; o += up((s / (size_t)threads + 2) * 4);
  L.lng = o; o += up((size_t)g.long_cap * long_bytes);
  L.end = o;
  return L;
}
// The two argument blocks of one batch item (DA = DetectArgs, TA = TailArgs, FX = BatchFixed of adsb_device.h): a canonical
// plan with the item's own threshold, its scratch at `sc` + L.*, its small words in fx.  One definition for the library and
// the emulator driver of the tests.
template <class DA, class TA, class FX>
inline void fill_batch_item(DA& a, TA& t, const Plan& pl, const BatchLay& L, char* sc, FX& fx, float thr, float scale, int sps,
                            bool long_aware, int lists) {
  a.data = pl.d_data; a.n = pl.n; a.in0_base = pl.in0_base; a.scan_lo = pl.scan_lo; a.scan_hi = pl.scan_hi;
  a.fall_hi = pl.fall_hi; a.dem_hi = pl.dem_hi; a.origin = pl.origin; a.chunk = L.g.chunk; a.thr = thr;
  a.prev_in0 = pl.prev_in0; a.scale = scale; a.sps = sps; a.end_is_call_end = pl.end_is_call_end;
  a.long_aware = long_aware ? 1 : 0; a.rec_cap = L.g.rec_cap; a.long_cap = L.g.long_cap;
  a.cands = (decltype(a.cands))(sc + L.cands); a.recs = (decltype(a.recs))(sc + L.recs); a.blk_count = fx.blk_count;
  a.blk_lastp = fx.blk_lastp; a.blk_flags = fx.blk_flags; a.longlist = (decltype(a.longlist))(sc + L.lng);
  a.long_count = &fx.long_count; a.long_lastp = &fx.long_lastp;
  t.cands = a.cands; t.recs = a.recs; t.blk_count = a.blk_count; t.blk_lastp = a.blk_lastp; t.blk_flags = a.blk_flags;
  t.blk_off = fx.blk_off; t.nblk = lists; t.rec_cap = L.g.rec_cap; t.long_count = a.long_count; t.long_lastp = a.long_lastp;
  t.sorted = (decltype(t.sorted))(sc + L.sorted); t.sorted_src = (decltype(t.sorted_src))(sc + L.src);
  t.seg_count = (decltype(t.seg_count))(sc + L.seg); t.sum = &fx.sum; t.host_sum = nullptr;
  t.out = (decltype(t.out))(sc + L.out); t.out_cap = (int)L.slots;
  t.gate_on = pl.gate ? 1 : 0; t.head_n = 0; t.gate = 63ll * sps; t.gate_long = (long long)(long_aware ? 119 : 63) * sps;
  t.prev_eob = pl.prev_eob_stream - pl.origin; t.seq = 0;
}

// framer.work() as GNU Radio calls it: the buffer IS in0 (N + 8*sps - 1 floats, history first).
inline Plan plan_framer_work(const void* d_in0, long long n_in0, long long N, long long nitems_written, int sps,
                             const FramerState& st) {
  const long long H = 8ll * sps;
  Plan p;
  p.mode = 1; p.d_data = d_in0; p.n = n_in0; p.in0_base = 0; p.scan_lo = 0; p.scan_hi = N; p.fall_hi = N;
  p.dem_hi = 0;                                          // framer does not slice bits
  p.origin = nitems_written - (H - 1);                   // framer.py:170
  p.prev_in0 = st.prev_in0; p.end_is_call_end = 1;
  p.prev_eob_stream = p.origin + st.prev_eob;
  p.gate = true;
  return p;
}

// State after a framer.work() call (framer.py:87,95,121-123,165,177-179).
//   flags bit0/bit1: the call saw >=1 rise / >=1 fall in in0[0:N]; lastp: in0 index of the last
//   paired pulse centre or `none`; last_kept: in0 index of the last accepted centre (n_kept > 0).
inline void framer_state_update(FramerState& st, float last_sample, long long N, int sps, unsigned flags,
                                long long lastp, long long none, int n_kept, long long last_kept) {
  st.prev_in0 = last_sample;                             // framer.py:87
  if ((flags & 1u) && (flags & 2u)) {                    // framer.py:95
    long long eob = st.prev_eob;
    if (n_kept > 0) eob = last_kept + 63ll * sps;        // framer.py:165
    if (lastp != none && lastp > eob) eob = -1;          // framer.py:121-123
    if (eob >= N) eob -= N;                              // framer.py:177-179
    st.prev_eob = eob;
  }
}

// One overlapped time shard of a canonical whole-stream call.  The buffer holds stream samples
// [origin, origin+n); this shard owns rises with stream offset in [own_lo, own_hi).
inline Plan plan_shard(int mode, const void* d, long long n, long long origin, long long own_lo, long long own_hi,
                       long long stream_len, int sps, int head_n = 0) {
  const long long H = 8ll * sps;
  const long long scan_end = stream_len - (H - 1);       // framer scans stream offsets [-(H-1), stream_len-(H-1))
  Plan p;
  p.mode = mode; p.d_data = d; p.n = n; p.origin = origin;
  p.in0_base = -(H - 1) - origin;
  long long lo = own_lo, hi = own_hi;
  if (lo <= 0 && origin == 0) lo = -(H - 1);
  if (hi > scan_end) hi = scan_end;
  p.scan_lo = lo - origin; p.scan_hi = hi - origin;
  if (p.scan_lo < p.in0_base) p.scan_lo = p.in0_base;
  const bool has_end = origin + n >= stream_len;
  p.fall_hi = has_end ? scan_end - origin : n;
  p.end_is_call_end = has_end ? 1 : 0;
  p.dem_hi = stream_len - origin;
  p.prev_in0 = 0.0f;
  p.prev_eob_stream = -(1ll << 61);
  p.gate = head_n > 0;                                   // gated with fresh state + whole head, or not gated at all
  p.head_n = head_n;
  return p;
}

// ---- receiver streams carried across batch calls (adsb_process_stream_batch*) ------------------------------------------
// A stream's calls are sequential in time, so one call is ONE overlapped time shard whose incoming end-of-burst state is
// known before the launch: the gate starts from the carried value (no head, no fix-up).  With the back halo B and the
// look-ahead F of adsb_shard_bounds, the call that appends samples [pos, pos + n) owns the rises of [pos - F, pos + n - F)
// -- the first owning call from the stream's start -- and the END item owns up to the end of the stream, with the
// end-of-call rules (framer.py:102-108, demod.py:82).  Offsets here are relative to the stream's first sample; `base` is
// what the records' offsets add to them.
constexpr long long kStreamUnbounded = 1ll << 60;        // STREAM_UNBOUNDED: plan_shard's stream_len of a stream that goes on
constexpr long long kStreamFreshEob = -(1ll << 61);      // the end-of-burst offset of a fresh stream: gates nothing
inline long long stream_back(int sps) { return 100 + 8ll * sps + 4; }          // B
inline long long stream_ahead(int sps) { return 256 + 121ll * sps; }           // F
inline long long stream_carry_max(int sps) { return stream_back(sps) + stream_ahead(sps) + 7; }
// A call's buffer starts at stream sample stream_origin(pos): B + F samples in front of the new chunk, rounded down to a
// multiple of 8 samples (16 bytes in every format), or at the stream's first sample.
inline long long stream_origin(long long pos, int sps) {
  const long long o = pos - stream_back(sps) - stream_ahead(sps);
  return o <= 0 ? 0 : o - o % 8;
}
// The stream's last samples that are kept on the device once it has consumed `pos` samples: exactly those the next call's
// buffer holds in front of its chunk -- all of a stream shorter than B + F, else B + F .. B + F + 7 of them.
inline long long stream_carry_len(long long pos, int sps) { return pos - stream_origin(pos, sps); }
struct StreamItem {
  long long origin;        // stream sample at the item's local index 0: a multiple of 8, so of 16 bytes in every format
  long long n_buf;         // the buffer holds stream samples [origin, pos + n): n_buf - n of them from the carry
  bool run;                // false: the item owns nothing (and is no END item): no pass, no records
  Plan plan;               // (d_data is the caller's to set when the buffer has its place)
};
inline StreamItem plan_stream_item(int mode, long long pos, long long n, bool end, long long base, long long eob, int sps) {
  const long long F = stream_ahead(sps);
  StreamItem it;
  it.origin = stream_origin(pos, sps);
  it.n_buf = pos + n - it.origin;
  const long long own_lo = pos - F, own_hi = end ? pos + n : pos + n - F;
  it.run = end ? it.n_buf > 0 : own_hi > 0;
  it.plan = plan_shard(mode, nullptr, it.n_buf, it.origin, own_lo, own_hi, end ? pos + n : kStreamUnbounded, sps, 0);
  it.plan.origin += base;
  it.plan.gate = true;
  it.plan.head_n = 0;
  it.plan.prev_eob_stream = eob;
  return it;
}
// The two copies of one stream item (SG = StreamStage, SV = StreamSave of adsb_device.h).  `carry_cur` holds the stream's last
// stream_carry_len(pos) samples (the buffer's head), `carry_next` takes those of pos + n; `buf` is the item's place in the
// staging buffer (16-byte aligned), `chunk` the caller's n new samples when the device has to copy them (else null: they
// are in place already).
template <class SG, class SV>
inline void fill_stream_copies(SG& g, SV& v, const StreamItem& it, long long pos, long long n, int sps, int bps, char* buf,
                               const char* carry_cur, char* carry_next, const void* chunk) {
  const long long head = stream_carry_len(pos, sps), keep = stream_carry_len(pos + n, sps);
  g.carry.src = carry_cur; g.carry.dst = buf; g.carry.bytes = head * bps;
  g.chunk.src = chunk; g.chunk.dst = buf + head * bps; g.chunk.bytes = chunk ? n * bps : 0;
  g.unit = bps; g.pad = 0;
  v.carry.src = buf + (it.n_buf - keep) * bps; v.carry.dst = carry_next; v.carry.bytes = keep * bps;
  v.unit = bps; v.pad = 0;
}
// What a stream item delivers and how its stream's state moves (ONE statement of both rules, for the library and the
// emulator driver).  A record is left out when its burst ends at or beyond the end of the item's buffer -- its last bits
// were sliced from samples that had not arrived: shard_post's rule (ADSB_SHARD_DROP_OVERLONG) -- and so is, by the kernel,
// a pulse still high there (Summary.flags bit 2): both are counted in *overlong.  *eob moves to the end of the last
// DELIVERED record's gate window (gate_window).
// off(r) / flags(r): a record's stream offset and its 16 flag bits.  Returns the number of records kept in dst (may be src).
template <class R, class Off, class Fl>
inline int stream_deliver(const R* src, int n, R* dst, const Plan& pl, unsigned sum_flags, int sps, Off off, Fl flags,
                          long long* eob, long long* overlong) {
  const long long buf_end = pl.origin + pl.n;
  int w = 0;
  if (sum_flags & 4u) ++*overlong;
  for (int i = 0; i < n; ++i) {
    const long long o = off(src[i]);
    const unsigned f = flags(src[i]);
    if ((f & ADSB_BURST_DEMOD) && o + 119ll * sps + sps / 2 >= buf_end) { ++*overlong; continue; }
    *eob = o + gate_window(f, sps);
    dst[w++] = src[i];
  }
  return w;
}

}  // namespace adsb

