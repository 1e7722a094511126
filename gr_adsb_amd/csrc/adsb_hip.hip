// adsb_hip.hip -- host side of libadsb_hip.so (C ABI in include/adsb_hip.h) for gfx950.
// Owns device memory, pinned staging and the launch sequence
//   k_detect (the one pass over the samples: centres AND their burst records)
//   -> k_order (long pulses, counts -> offsets, words in stream order) -> k_resolve -> k_count -> k_compact (+ summary to the host)
// There is deliberately no CPU implementation of the path in this library.
//
// The library reads no environment variable.
#include <hip/hip_runtime.h>

#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "adsb_shared.h"
#include "adsb_dedup.h"
#include "adsb_mlat.h"
#include "adsb_mlat_rule.h"
#include "adsb_mlat_track.h"

#include "adsb_env_hip.h"

#include "adsb_device.h"
#include "adsb_plan.h"
#include "adsb_seam.h"
#include "adsb_softfec.h"
#include "adsb_softfec_batch.h"
#include "../../include/adsb_hip.h"

using namespace adsb;

static_assert(sizeof(adsb_burst) == 32 && sizeof(Rec) == 32, "record layout");
static_assert(sizeof(adsb_decoded) == sizeof(DecRow) && offsetof(adsb_decoded, latitude) == offsetof(DecRow, latitude) &&
              offsetof(adsb_decoded, num_msgs) == offsetof(DecRow, num_msgs), "decoded row layout");

namespace {

// Owners: whatever a context creates -- device memory, page-locked memory, streams, events -- is held by a member that
// releases it when the context is deleted (adsb_destroy synchronises, then `delete c`): a new member needs no line anywhere
// else.  Move-only; no allocation and no HIP call outside create / grow / release; `.p` is a plain pointer read.
template <class P, auto Release>
struct Owned {
  P p = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : p(o.p) { o.p = nullptr; }
  ~Owned() { (void)release(); }
  hipError_t release() {
    const hipError_t e = p ? Release(p) : hipSuccess;
    p = nullptr;
    return e;
  }
  operator P() const { return p; }
  P operator->() const { return p; }
};
template <class T> using DevPtr = Owned<T*, hipFree>;         // device memory of a fixed size
template <class T> using PinnedPtr = Owned<T*, hipHostFree>;  // page-locked host memory of a fixed size
using Stream = Owned<hipStream_t, hipStreamDestroy>;          // a queue the context created (never a caller's: adsb_set_stream)
using Event = Owned<hipEvent_t, hipEventDestroy>;
// ... and memory that grows on demand (ensure / ensure_pinned)
template <auto Release>
struct Buf : Owned<void*, Release> {
  size_t cap = 0;
  hipError_t release() { cap = 0; return Owned<void*, Release>::release(); }
};
using DevBuf = Buf<hipFree>;
using PinnedBuf = Buf<hipHostFree>;

// d_misc layout: [0] int long_count, [8] u64 long_lastp, [16] OrderAcc (k_order's accumulator), [64] Summary
struct Misc {
  int long_count;
  int pad;
  unsigned long long long_lastp;
  OrderAcc acc;
  char fill[32];
  Summary sum;
};
static_assert(sizeof(OrderAcc) == 16, "Misc layout");

// Everything one in-flight call needs on the device and in pinned host memory.  Several slots let call i+1
// run on the GPU while the records of call i travel over PCIe (adsb_submit_* / adsb_wait), and -- host-fed -- while
// the samples of call i+2 travel the other way.
struct Slot {
  DevBuf d_cands, d_recs, d_sorted, d_sorted_src, d_out, d_seg, d_blk_count, d_blk_lastp, d_blk_flags, d_blk_off, d_long, d_misc;
  DevBuf d_in;                   // host-fed submissions: this call's samples (adsb_submit_format_host)
  DevBuf d_ratio;                // ADSB_FLAG_CONFIDENCE: [n_kept][112] bit1/bit0 ratios
  PinnedPtr<Summary> h_sum;
  PinnedBuf h_out;               // burst records of the finished call
  PinnedBuf h_ratio;             // confidence ratios of the finished call
  DevBuf d_soft;                 // ADSB_FLAG_FEC_SOFT: one adsb_soft_fix per list slot (adsb_softfec.hip writes one per delivered record)
  PinnedBuf h_soft;              // ... and the rows of the finished call's records
  Event done, ev0, ev1, det_done, h2d_done;
  Stream stream;                 // this slot's own in-order queue: a SUBMITTED pass runs on it from k_detect to k_compact (see enqueue)
  hipStream_t ds = nullptr;      // the stream this pass's k_detect was queued on ...
  hipStream_t cs = nullptr;      // ... and the one its tail, its summary and its record copy run on (the same, or behind an event)
  bool busy = false;
  bool direct = false;           // small pass: k_compact writes the records straight into h_out (no device->host copy)
  bool fused = false;            // ... and the whole pass is ONE launch (k_pass_small)
  int host_cap = 0;              // mid-size pass: k_compact stores the first host_cap records into h_out as well (see enqueue)
  bool is_shard = false;
  bool submitted = false;        // queued by adsb_submit_* / the sharded driver (other passes may be in flight beside it)
  bool ev1_valid = false;
  bool h2d_pending = false;      // host-fed submission: the upload's event has to be waited for by the k_detect stream
  int seq = 0;                   // direct passes: the number the kernel stores into h_sum->pad_ when everything is out
  unsigned long long air_pass = 0;   // ADSB_FLAG_AIRCRAFT_TABLE: this pass's number << 32, kept when the pass is re-run
  bool air_keep = false;             // ... set while finish() re-runs the pass
  PinnedBuf h_dec;                   // ADSB_FLAG_DECODE: rows of the pass's delivered records (adsb_last_decoded)
  bool polled = false;           // ... and finish() polls for instead of waiting for an event
  Plan plan{};
  DetectArgs args{};
  int grid = 0, nlists = 0, rec_cap = 0;
  long long tot = 0, ntiles = 0, chunk = 0, span = 0;
  int32_t nres = 0;
};

// adsb_process_batch*: the context's buffers: they grow on demand like a slot's and are PER ITEM (an item's records have to outlive
// its workgroup: k_batch_pack gathers them), so their size follows the batch, not the device -- see run_batch
struct BatchBufs {
  DevBuf d_scratch;              // per item: cands, sorted, recs, out, sorted_src, seg_count, long-pulse list
  DevBuf d_fixed;                // BatchFixed[n_items]
  DevBuf d_da, d_ta, d_kept;     // the two argument tables and k_batch's verdict per item
  DevBuf d_packed, d_tot;        // the dense record list and its Summary (n_kept = number of records: k_fec's bound)
  DevBuf d_in;                   // adsb_process_batch: the device copy of every item
  PinnedBuf h_tab;               // the tables as the host builds them
  PinnedBuf h_first;             // device-visible: first[n_items + 1], then kept[n_items]
  PinnedBuf h_out;               // device-visible: the dense list (its head straight from k_batch_pack)
  // ADSB_FLAG_FEC_SOFT_BATCH (adsb_softfec_batch.hip): the items' samples as a table of its own (the units share no type), one
  // adsb_soft_fix per slot of the dense list, and the rows of the finished pass's records
  DevBuf d_soft_items, d_soft_rows;
  PinnedBuf h_soft_rows;
};

// adsb_process_stream_batch*: the receiver streams of a context (adsb_streams_open).  Host state per stream, its last
// samples on the device in two slots of the widest format's size, and the buffers of one call.
struct StreamState {
  long long pos = 0;                   // samples consumed
  long long eob = kStreamFreshEob;     // carried end-of-burst offset (record offsets: base included)
  long long base = 0;                  // what the records' offsets add to the stream's sample index
  long long overlong = 0;              // pulses / bursts left out because they ran past a call's buffer
  int cur = 0;                         // the carry slot that holds the stream's last samples
  int fmt = -1;                        // the format the stream started with (-1: fresh)
};
// fresh again (adsb_stream_reset, adsb_reset): the base stays, the overlong count starts over.  (An END item leaves the
// stream fresh too, but keeps its count.)
inline void stream_make_fresh(StreamState& s) { s.pos = 0; s.eob = kStreamFreshEob; s.overlong = 0; s.fmt = -1; }
struct StreamBufs {
  std::vector<StreamState> st;
  size_t slot_bytes = 0;         // one carry slot: stream_carry_max(sps) complex64 samples, whole 256-byte lines
  DevBuf d_carry;                // [n_streams][2][slot_bytes]
  DevBuf d_stage;                // this call's item buffers [stream carry | new chunk], each on a 256-byte boundary
  DevBuf d_tab;                  // StreamStage[n_items], StreamSave[n_items]
  PinnedBuf h_tab;               // ... as the host builds them
  PinnedBuf h_status;            // device-visible: StreamStatus[n_items] (k_stream_save)
};

// ADSB_FLAG_STREAM_DECODE: the decoders of the context's streams (adsb_device.h: the k_fleet_* kernels).  Host state per
// stream (start timestamp, generation, the slots and planes it holds), the store, and the buffers of one call's decode step.
struct FleetDec {
  bool open = false;
  int all = 1;                                  // msg_filter "All Messages"
  std::vector<double> start;
  std::vector<unsigned> gen;
  std::vector<long long> slots, planes;         // live, per stream
  long long cap = 0;                            // slots of the store
  long long used = 0;                           // slots taken since the store was built (those of reset streams included)
  long long live_slots = 0, live_planes = 0, grows = 0;
  unsigned long long call = 0;                  // number of the next delivered call with records (ordering keys: number << 32 | position)
  DevBuf d_store;                               // keys[cap] | ann[cap] | planes[cap] (| last_seen[cap]: ADSB_FLAG_PLANE_AGES)
  DevBuf d_ages;                                // adsb_stream_planes_expire: cutoffs[n_streams] | removed[n_streams]; _seen: last_seen[n]
  DevBuf d_recs, d_items, d_cnt, d_keys, d_sorted, d_tmp, d_ts, d_rows, d_gen;
  DevBuf d_snap;                                // adsb_stream_planes: generations | selection bitmap | selection list | first[] | count, error
  DevBuf d_merged;                              // adsb_stream_planes_merged: the adsb_merged entries beside d_rows
  DevBuf d_shared;                              // ADSB_FLAG_STREAM_DECODE_SHARED: the time order's buffers of one call (SharedBufs)
  PinnedBuf h_recs, h_rows, h_items, h_cnt;
  PinnedBuf h_shared, h_order;                  // ... the items' first[] | start[] on their way up, order[] of the last delivered call
  PinnedBuf h_order_next;                       // ... and where a call's order[] arrives: the two change places once the call is delivered
  int32_t n_rows = 0;                           // rows of the last delivered call
  // ADSB_FLAG_STREAM_DEDUP (adsb_dedup.hip): the carry is d_carry[cur][off .. off + cnt), entries of 32 bytes in time order.
  // A call merges into the other buffer and changes cur / off / cnt / hi only once it is delivered.
  struct Dedup {
    double window = 0.002, horizon = 1.0, hi = 0;
    int cur = 0, off = 0, cnt = 0;
    long long duplicates = 0;
    bool delivered = false;                     // a call with records since the decoder was last fresh
    DevBuf d_carry[2];
    DevBuf d_call;                              // one call's entries[n] | dup[n] | item_stream[n_items]
    PinnedBuf h_dup, h_dup_next;                // dup[] of the last delivered call / where a call's arrives (as h_order)
    void fresh() { hi = 0; off = cnt = 0; duplicates = 0; delivered = false; }
  } dd;
  // adsb_stream_mlat (adsb_mlat.hip): the receivers' ECEF positions (NaN: none set) -- not decoder state: only fleet_open and
  // fleet_close touch them -- and one call's work buffer (adsb_mlat.h: Layout; adsb_stream_mlat_rule's damped path carves the
  // same buffer by adsb_mlat_rule.h: layout_rule) with the pinned memory its counts come down to
  std::vector<double> rx;
  DevBuf d_mlat;
  PinnedBuf h_mlat;
  // the MLAT track store (adsb_mlat_track.hip): d_rows[cur][0 .. n) in ascending icao; a call merges into the other buffer
  // and changes cur / n once its counts are down and in range.  Not decoder state: only fleet_close and
  // adsb_stream_mlat_tracks_reset forget it.  d_work: one call's buffer (adsb_mlat_track.h: Layout); h_cnt: where counts come down.
  struct Tracks {
    int cur = 0, n = 0;
    DevBuf d_rows[2], d_work;
    PinnedBuf h_cnt;
  } trk;
};
constexpr long long kFleetMinCap = 256, kFleetDefaultCap = 1ll << 16, kFleetMaxCap = 1ll << 27;    // (slot index 2^28 - 1 would sort with kDecNoKey)
constexpr size_t kFleetSlotBytes = 16 + sizeof(Plane);
static_assert(sizeof(Rec) == adsb_shared_host::kRecBytes && sizeof(DecRow) == adsb_shared_host::kRowBytes,
              "adsb_shared.hip moves records and rows as opaque words of these sizes");
static_assert(offsetof(Rec, w) == 0 && kSortTile == adsb_shared_host::kSortTile, "a record's offset is its word 0; one sort tile");
static_assert(sizeof(Rec) == adsb_dedup_host::kRecBytes && sizeof(DecRow) == adsb_dedup_host::kRowBytes && offsetof(DecRow, port) == 0 &&
              ADSB_DEC_DUPLICATE == 4u && kDemod == ADSB_BURST_DEMOD && kLongFmt == ADSB_BURST_LONG,
              "adsb_dedup.hip reads a record's flags in word 3 and writes a row's port in byte 0");
static_assert(sizeof(adsb_mlat_fix) == adsb_mlat_host::kFixBytes && offsetof(adsb_mlat_fix, bits) == 48 && offsetof(adsb_mlat_fix, flags) == 62 &&
              offsetof(adsb_mlat_fix, icao) == 64 && offsetof(adsb_mlat_fix, first) == 84 && adsb_mlat_host::kEntBytes == adsb_dedup_host::kEntBytes &&
              ADSB_BURST_LONG == 64u, "adsb_mlat.hip writes adsb_mlat_fix rows and reads the carry's entries");
// ADSB_FLAG_STREAM_DECODE_SHARED: d_shared carved for a call of n records in n_items items, every part on a 256-byte boundary
struct SharedBufs {
  unsigned long long *keys = nullptr, *keys_tmp = nullptr;
  double *ts = nullptr, *ts_sorted = nullptr;
  Rec* recs = nullptr;                          // the time-ordered list the decode step runs on
  DecRow* rows = nullptr;                       // ... and its rows
  unsigned *vals = nullptr, *vals_tmp = nullptr, *hist = nullptr;
  int *order = nullptr, *first = nullptr;
  double* start = nullptr;
  SharedBufs() = default;                       // a context without the flag: nothing
  // the parts' offsets in bytes, in the members' order -> the size of the whole
  static size_t layout(size_t n, size_t n_items, size_t off[12]) {
    const size_t part[12] = {n * 8, n * 8, n * 8, n * 8, n * sizeof(Rec), n * sizeof(DecRow), n * 4, n * 4,
                             adsb_shared_host::sort_hist_bytes((int)n), n * 4, (n_items + 1) * sizeof(int), n_items * sizeof(double)};
    size_t at = 0;
    for (int k = 0; k < 12; ++k) { off[k] = at; at += (part[k] + 255) & ~(size_t)255; }
    return at;
  }
  static size_t bytes(size_t n, size_t n_items) { size_t off[12]; return layout(n, n_items, off); }
  // base: device memory of bytes(n, n_items)
  SharedBufs(void* base, size_t n, size_t n_items) {
    size_t off[12];
    layout(n, n_items, off);
    char* const b = (char*)base;
    keys = (unsigned long long*)(b + off[0]); keys_tmp = (unsigned long long*)(b + off[1]);
    ts = (double*)(b + off[2]); ts_sorted = (double*)(b + off[3]);
    recs = (Rec*)(b + off[4]); rows = (DecRow*)(b + off[5]);
    vals = (unsigned*)(b + off[6]); vals_tmp = (unsigned*)(b + off[7]); hist = (unsigned*)(b + off[8]);
    order = (int*)(b + off[9]); first = (int*)(b + off[10]); start = (double*)(b + off[11]);
  }
};

}  // namespace

// Host threads that copy a pageable source into the pinned staging ring of a host-fed submission: one host core moves
// ~10 GB/s, the DMA behind it 57 -- so the copy of every chunk is split over a few threads (created on the first pageable
// submission, parked on a condition variable in between).
struct CopyPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  const char* src = nullptr;
  char* dst = nullptr;
  size_t bytes = 0;
  unsigned gen = 0;
  int pending = 0;
  bool stop = false;
  int nthreads = 0;      // workers besides the caller
  cpu_set_t cpus;        // the host cpus local to the context's GPU (NUMA node of its PCI device); workers run there
  bool have_cpus = false;

  static void slice(size_t bytes, int parts, int i, size_t* lo, size_t* hi) {
    const size_t per = ((bytes / (size_t)parts) + 4095) & ~(size_t)4095;
    *lo = per * (size_t)i < bytes ? per * (size_t)i : bytes;
    *hi = (i == parts - 1) ? bytes : (*lo + per < bytes ? *lo + per : bytes);
  }
  void worker(int id) {
    unsigned seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(m);
      cv_job.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      const char* s_ = src; char* d_ = dst; const size_t b_ = bytes;
      lk.unlock();
      size_t lo, hi;
      slice(b_, nthreads + 1, id + 1, &lo, &hi);
      if (hi > lo) memcpy(d_ + lo, s_ + lo, hi - lo);
      lk.lock();
      if (--pending == 0) cv_done.notify_one();
    }
  }
  void start(int n) {
    nthreads = n;
    for (int i = 0; i < n; ++i) {
      th.emplace_back([this, i] { worker(i); });
      // the copy of a pageable source into the pinned ring is bound by host memory bandwidth: keep it on the socket the
      // ring lives on and the GPU hangs off (best effort: an error leaves the thread where the scheduler puts it)
      if (have_cpus) (void)pthread_setaffinity_np(th.back().native_handle(), sizeof(cpus), &cpus);
    }
  }
  // blocking: returns when all of [src, src + bytes) is in dst
  void copy(char* d_, const char* s_, size_t b_) {
    if (nthreads == 0 || b_ < ((size_t)1 << 20)) { memcpy(d_, s_, b_); return; }
    {
      std::lock_guard<std::mutex> lk(m);
      src = s_; dst = d_; bytes = b_; pending = nthreads; ++gen;
    }
    cv_job.notify_all();
    size_t lo, hi;
    slice(b_, nthreads + 1, 0, &lo, &hi);
    memcpy(d_ + lo, s_ + lo, hi - lo);
    std::unique_lock<std::mutex> lk(m);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv_job.notify_all();
    for (std::thread& t : th) t.join();
  }
};

// One context.  Four rules of its host side are each kept in one place:
//   * what it creates it releases: every buffer, stream and event is an owner member (DevBuf, PinnedBuf, DevPtr, PinnedPtr,
//     Stream, Event, the copy pool); adsb_destroy only synchronises and deletes;
//   * a call that fails releases its pipeline slot: enqueue() and finish() do, no caller does;
//   * nothing runs while a submitted call is pending: require_idle();
//   * a per-record step gets step_grid(n, per) workgroups.
// claim_and_enqueue() hands the next slot to a submitted pass, requeue_grown() re-runs a pass whose lists overflowed.
struct adsb_ctx {
  int device = 0;
  double fs = 0;
  int sps = 0;
  float thr = 0;
  uint32_t flags = 0;
  // Queues.  A SUBMITTED pass (adsb_submit_*, the sharded driver) runs on its pipeline slot's own stream, k_detect and its
  // tail back to back: passes in different slots share nothing, so the hardware overlaps them as resources allow -- the
  // tail of pass i runs beside k_detect of pass i+1, and k_detect i+1 fills the CUs k_detect i drains from -- without one
  // event between them (round 5; until then: k_detect of every pass on `stream`, every tail on `tail_stream` behind an
  // event per pass: 9 us of the 27 us of host time a submission cost, tools/micro/launch_cost.hip).  A BLOCKING call runs
  // alone, on `stream`, as one queue.  A caller-owned stream (adsb_set_stream) keeps the old arrangement: k_detect on it,
  // tails on `tail_stream`; so do timed passes and passes over more than 4 GiB, with the slot streams in those roles (enqueue).
  // Few streams on purpose: the runtime multiplexes streams onto four hardware queues by default, and two streams that share
  // one serialise.  A context of its own uses three (the slots') plus the upload stream of host-fed submissions;
  // the record copy of a finished pass goes onto that pass's own -- by then idle -- stream.
  hipStream_t stream = nullptr;       // compute stream of the blocking entry points: slot 0's stream, or the caller's (adsb_set_stream)
  Stream copy_stream;                 // caller-owned compute stream only: device -> pinned host result copies
  Stream tail_stream;                 // caller-owned compute stream only: everything after k_detect
  // adsb_wait_for_event: the caller's events the NEXT pass has to wait for (applied to the stream its first kernel runs on)
  static constexpr int kMaxExt = 4;
  hipEvent_t ext_ev[kMaxExt] = {nullptr, nullptr, nullptr, nullptr};
  int n_ext = 0;
  Stream h2d_stream;                  // host-fed submissions: sample uploads, back to back on their own stream
  Stream d2h_stream;                  // record copies of in-line passes while slot 2's stream holds an overlapped pass (created on first use)
  bool split_tail = false;
  bool own_stream = false;
  int n_cu = 256;
  int bpc[ADSB_FMT_COUNT] = {4, 4, 4, 4, 4};  // resident k_detect workgroups per CU (occupancy query), per input format
  // Unused dynamic LDS per k_detect workgroup = how many workgroups share a CU (28.3 KB static: five fit; 6 KB of padding
  // would lift a workgroup over the 32 KB that five per CU allow).  Measured per format on MI355X (tools/r3_variants.sh,
  // 2^30 samples): five per CU for every format since round 4 -- float |IQ|^2 ran best with four until the SGPR spills went
  // (five: +1.3 % pipelined, 0.78 instead of 0.72 of its roofline isolated; profiles/r04_ab_workgroups_per_cu.txt); three:
  // -24 % for the 8-bit formats.  Six would need 1.4 KB less LDS per workgroup: a 256-entry rise list worked off in two
  // halves was built and measured -- six workgroups gave the 8-bit formats +5 %, the second code path took 4 % back.
  unsigned det_dyn_lds[ADSB_FMT_COUNT] = {0, 0, 0, 0, 0};
  unsigned lds_beside[ADSB_FMT_COUNT] = {0, 0, 0, 0, 0};    // LDS a CU has left beside its resident k_detect workgroups
  // integer IQ component -> float32 multiplier per format (adsb_set_format_scale); unused for the float formats
  float scale[ADSB_FMT_COUNT] = {1.0f, 1.0f, 1.0f / 32768.0f, 1.0f / 128.0f, 1.0f / 255.0f};
  FramerState st;       // framer.py:54,57
  Slot slot[ADSB_MAX_IN_FLIGHT];
  int next_slot = 0;
  int last_slot = 0;
  DevBuf d_in;            // device copy of the host input of the blocking entry points
  int rec_cap_shift = 0;  // rec_cap multiplier (grows on overflow)
  PinnedBuf h_stage;         // staging for pageable inputs of the blocking entry points
  PinnedBuf h_dm;            // scratch of adsb_demod_work: tag positions in, bits / ok / ratio out
  // ADSB_FLAG_FEC_SOFT: the rule (adsb_set_soft_fec), and where adsb_last_soft finds the rows of the last adsb_demod_work
  // (in h_dm) when that was the context's last call
  adsb_soft_fec_rule soft_rule{8, 3, 0.0f, 0u};
  const adsb_soft_fix* soft_dm = nullptr;
  int32_t soft_dm_n = 0;
  // ADSB_FLAG_FEC_SOFT_BATCH: the per-call switch of the ordinary pass -- set only while batch_core runs an item through
  // enqueue / finish, so every other entry point of such a context does what it does without the flag -- and the rows of the
  // last delivered batch call in the order of its out[] (adsb_batch_last_soft)
  bool soft_fallback = false;
  std::vector<adsb_soft_fix> batch_soft;
  static constexpr int kRing = 4;
  PinnedPtr<void> h_ring[kRing];   // chunks for pageable host-fed submissions
  Event ring_done[kRing];
  bool ring_used[kRing] = {false, false, false, false};
  unsigned ring_k = 0;
  // NUMA placement of the host side (adsb_numa_info): the node and cpus local to the GPU's PCI device, from sysfs
  int numa_node = -1;
  char pci_bdf[32] = {0};
  char cpulist[256] = {0};
  cpu_set_t local_cpus;
  bool have_local_cpus = false;
  std::unique_ptr<CopyPool> pool;   // host copy threads of the pageable path (adsb_set_copy_threads; created on first use)
  int copy_threads = -1;       // -1 = default
  adsb_stats stats{};
  // per-launch k_detect durations of the timed calls (ADSB_FLAG_TIMING), a ring of the last kHist: adsb_detect_history
  static constexpr int kHist = 4096;
  std::vector<float> det_hist;
  uint64_t det_hist_n = 0;
  // ADSB_FLAG_AIRCRAFT_TABLE: 2^24 first-announcement keys, the step state, and the event behind the last table step queued
  DevPtr<unsigned long long> d_air;
  DevPtr<AirState> d_air_st;
  Event air_ev;
  unsigned long long air_next = 0;    // number of the next published pass (table keys: number << 32 | position)
  // ADSB_FLAG_DECODE: the plane state of every address, the epoch that marks an entry valid, the decoder's settings, and
  // the sort's buffers (one decode step runs at a time: the table step's event chain orders them)
  DevPtr<Plane> d_planes;
  unsigned dec_epoch = 1;
  int dec_all = 1;
  double dec_start = 0;
  DevBuf d_dec_keys, d_dec_sorted, d_dec_tmp;
  PinnedBuf h_pdu;                    // adsb_decode_pdus' staging (device-visible)
  DevBuf d_snap_cnt, d_snap_rows;     // adsb_planes: the chunks' counts / first rows, and the snapshot's rows
  DevPtr<long long> d_seen;           // ADSB_FLAG_PLANE_AGES: 2^24 last_seen clocks beside d_planes (adsb_device.h: plane ages)
  DevBuf d_snap_seen;                 // adsb_planes_seen: the snapshot's last_seen
  BatchBufs bt;                       // adsb_process_batch*
  StreamBufs sb;                      // adsb_process_stream_batch*
  FleetDec fd;                        // ... and their decoders (ADSB_FLAG_STREAM_DECODE)
  char err[256] = {0};
  __attribute__((visibility("hidden"))) ~adsb_ctx() = default;   // (the library's exported names stay its C entry points)
};

namespace {

// one polite iteration of a host spin loop
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::this_thread::yield();
#endif
}

int fail(adsb_ctx* c, int code, const char* what, hipError_t he = hipSuccess) {
  if (c) {
    if (he != hipSuccess) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(he));
    else snprintf(c->err, sizeof(c->err), "%s", what);
  }
  return code;
}

#define HIPCHK(c, call)                                   \
  do {                                                    \
    hipError_t e_ = (call);                               \
    if (e_ != hipSuccess) return fail((c), -EIO, #call, e_); \
  } while (0)

int ensure(adsb_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return 0;
  const hipError_t e = b.release();
  if (e != hipSuccess) return fail(c, -EIO, "hipFree(b.p)", e);
  size_t want = bytes + bytes / 4 + 256;
  HIPCHK(c, hipMalloc(&b.p, want));
  b.cap = want;
  return 0;
}

// Page-locked host memory on the NUMA node of the context's GPU: the calling thread's memory policy is set to prefer that
// node for the duration of the allocation (raw set_mempolicy: no libnuma in the image) and hipHostMallocNumaUser tells HIP
// to honour it.  Without a known node (numa_node < 0: single-socket host, or sysfs not visible) a plain allocation.
constexpr int kMpolDefault = 0, kMpolPreferred = 1;
// `coherent`: the buffer is read by the HOST while the kernel that writes it may still be running (the polled summary and
// the records of a one-workgroup pass): asked for explicitly as fine-grained memory (hipHostMallocCoherent) instead of
// relying on the runtime's default / HIP_HOST_COHERENT.
hipError_t host_alloc_near(adsb_ctx* c, void** p, size_t bytes, bool coherent = false) {
  const unsigned co = coherent ? hipHostMallocCoherent : 0u;
  if (!c || c->numa_node < 0 || c->numa_node >= 1024) {
    hipError_t e0 = hipHostMalloc(p, bytes, hipHostMallocDefault | co);
    if (e0 != hipSuccess && co) { (void)hipGetLastError(); e0 = hipHostMalloc(p, bytes, hipHostMallocDefault); }
    return e0;
  }
  unsigned long mask[16] = {0}, old_mask[16] = {0};
  mask[c->numa_node / (8 * sizeof(unsigned long))] |= 1ul << (c->numa_node % (8 * sizeof(unsigned long)));
  // the caller's own policy is put back afterwards (whatever it was)
  int old_mode = kMpolDefault;
  const bool have_old = syscall(SYS_get_mempolicy, &old_mode, old_mask, sizeof(old_mask) * 8, nullptr, 0) == 0;
  const long rc = syscall(SYS_set_mempolicy, kMpolPreferred, mask, sizeof(mask) * 8);
  hipError_t e = hipHostMalloc(p, bytes, (rc == 0 ? hipHostMallocNumaUser : hipHostMallocDefault) | co);
  if (e != hipSuccess && co) {                       // (a runtime that refuses the combination: placement first)
    (void)hipGetLastError();
    e = hipHostMalloc(p, bytes, rc == 0 ? hipHostMallocNumaUser : hipHostMallocDefault);
  }
  if (rc == 0) {
    if (!have_old || old_mode == kMpolDefault || syscall(SYS_set_mempolicy, old_mode, old_mask, sizeof(old_mask) * 8) != 0)
      (void)syscall(SYS_set_mempolicy, kMpolDefault, nullptr, 0);
  }
  if (e != hipSuccess && rc == 0) { (void)hipGetLastError(); e = hipHostMalloc(p, bytes, hipHostMallocDefault); }
  return e;
}

// "0-63,128-191" -> cpu set
bool parse_cpulist(const char* sl, cpu_set_t* set) {
  CPU_ZERO(set);
  int any = 0;
  const char* p = sl;
  while (*p) {
    char* e = nullptr;
    long a = strtol(p, &e, 10);
    if (e == p) break;
    long b = a;
    p = e;
    if (*p == '-') { b = strtol(p + 1, &e, 10); if (e == p + 1) break; p = e; }
    for (long k = a; k <= b && k < CPU_SETSIZE; ++k) { if (k >= 0) { CPU_SET((int)k, set); ++any; } }
    if (*p == ',') ++p; else break;
  }
  return any > 0;
}

bool read_line(const char* path, char* out, size_t cap) {
  FILE* f = fopen(path, "r");
  if (!f) return false;
  const bool ok = fgets(out, (int)cap, f) != nullptr;
  fclose(f);
  if (ok) { size_t n = strlen(out); while (n && (out[n - 1] == '\n' || out[n - 1] == ' ')) out[--n] = 0; }
  return ok;
}

// numa_node / local_cpulist of the GPU's PCI device (/sys/bus/pci/devices/<bdf>/): which host memory and which cpus are
// local to it.  Best effort: a container may hide sysfs, a single-socket host reports node -1 or 0.
void probe_numa(adsb_ctx* c) {
  char bdf[32] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), c->device) != hipSuccess) { (void)hipGetLastError(); return; }
  for (char* q = bdf; *q; ++q) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');      // sysfs spells it in lower case
  snprintf(c->pci_bdf, sizeof(c->pci_bdf), "%s", bdf);
  char path[128], line[256];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  if (read_line(path, line, sizeof(line))) c->numa_node = atoi(line);
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bdf);
  if (read_line(path, line, sizeof(line)) && line[0]) {
    snprintf(c->cpulist, sizeof(c->cpulist), "%s", line);
    c->have_local_cpus = parse_cpulist(line, &c->local_cpus);
  }
}

int ensure_pinned(adsb_ctx* c, PinnedBuf& b, size_t bytes, bool coherent = false) {
  if (bytes <= b.cap) return 0;
  const hipError_t e = b.release();
  if (e != hipSuccess) return fail(c, -EIO, "hipHostFree(p)", e);
  size_t want = bytes + bytes / 4 + 4096;
  HIPCHK(c, host_alloc_near(c, &b.p, want, coherent));
  b.cap = want;
  return 0;
}

// Workgroups of a per-record step: ceil(n / per), at least one, at most kMaxStepGrid.  (adsb_decode_pdus and adsb_demod_work
// had no floor of one: they return before the launch when n == 0, so the value is the same.)
constexpr long long kMaxStepGrid = 2048;
unsigned step_grid(long long n, int per) { return (unsigned)std::max(1ll, std::min(kMaxStepGrid, (n + per - 1) / per)); }

// Nothing runs while a submitted call is pending: -EBUSY with the caller's text (on `err_to` where that is another context).
const char* const kCallPending = "a submitted call is still pending (adsb_wait first)";
int require_idle(adsb_ctx* c, const char* text, adsb_ctx* err_to = nullptr) {
  for (const Slot& sl : c->slot) if (sl.busy) return fail(err_to ? err_to : c, -EBUSY, text);
  return 0;
}

// one instantiation of every sample-reading kernel per input format (ADSB_FMT_*)
#define ADSB_BY_MODE(mode, F, ...)            \
  switch (mode) {                             \
    case 0: F<0>(__VA_ARGS__); break;         \
    case 1: F<1>(__VA_ARGS__); break;         \
    case 2: F<2>(__VA_ARGS__); break;         \
    case 3: F<3>(__VA_ARGS__); break;         \
    default: F<4>(__VA_ARGS__); break;        \
  }

// k_detect is instantiated per input format and per samples-per-chip of the common rates (2, 4, 8, 20 Msps: the
// preamble taps become immediate offsets); any other even rate runs the run-time-stride instance
template <int KMODE>
void launch_detect_k(hipStream_t st, unsigned dyn, const DetectArgs& a, int grid) {
  switch (a.sps) {
    case 2: hipLaunchKernelGGL((k_detect<KMODE, 1>), dim3(grid), dim3(64 * det_waves(KMODE)), dyn, st, a); break;
    case 4: hipLaunchKernelGGL((k_detect<KMODE, 2>), dim3(grid), dim3(64 * det_waves(KMODE)), dyn, st, a); break;
    case 8: hipLaunchKernelGGL((k_detect<KMODE, 4>), dim3(grid), dim3(64 * det_waves(KMODE)), dyn, st, a); break;
    case 20: hipLaunchKernelGGL((k_detect<KMODE, 10>), dim3(grid), dim3(64 * det_waves(KMODE)), dyn, st, a); break;
    default: hipLaunchKernelGGL((k_detect<KMODE, 0>), dim3(grid), dim3(64 * det_waves(KMODE)), dyn, st, a); break;
  }
}
// a power of two whose square, times any integer below 2^15, is an exact float32: what the int8 dot-product instance needs
bool scale_is_pow2(float s) {
  int e = 0;
  const float m = frexpf(s, &e);
  return m == 0.5f && e > -50 && e < 50;
}
template <int MODE>
void launch_detect(adsb_ctx* c, hipStream_t st, const DetectArgs& a, int grid) {
  const unsigned dyn = c->det_dyn_lds[MODE];
  // int8 IQ with a power-of-two scale (x / 128 and the like): the instance whose tile loop squares with v_dot4_i32_i8
  if (MODE == ADSB_FMT_SC8 && scale_is_pow2(a.scale)) launch_detect_k<kModeSc8Pow2>(st, dyn, a, grid);
  // uint8 IQ with a power-of-two scale ((u8 - 127.5) / 128 and the like): the same for offset-binary bytes
  else if (MODE == ADSB_FMT_CU8 && scale_is_pow2(a.scale)) launch_detect_k<kModeCu8Pow2>(st, dyn, a, grid);
  else launch_detect_k<MODE>(st, dyn, a, grid);
}
template <int MODE>
unsigned detect_static_lds() {
  hipFuncAttributes at;
  if (hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_detect<MODE, 0>)) != hipSuccess) { (void)hipGetLastError(); return 32768u; }
  return (unsigned)at.sharedSizeBytes;
}
template <int MODE>
int detect_occupancy(unsigned dyn) {
  // (the instances of one format differ only in tap addressing: the same resources decide)
  int nb = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_detect<MODE, 0>, 64 * det_waves(MODE), dyn);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
  return nb;
}
template <int MODE>
void launch_order(hipStream_t st, int grid, unsigned dyn, const DetectArgs& a, int nblk, unsigned long long* sorted, unsigned* sorted_src,
                  Summary* sum, OrderAcc* acc) {
  hipLaunchKernelGGL((k_order<MODE>), dim3(grid), dim3(kThreads), dyn, st, a, nblk, sorted, sorted_src, sum, acc);
}
template <int MODE>
void launch_tail_small(hipStream_t st, const DetectArgs& a, const TailArgs& t) {
  hipLaunchKernelGGL((k_tail_small<MODE>), dim3(1), dim3(kThreads), 0, st, a, t);
}
// the whole small pass in one launch (|IQ|^2 float input, one workgroup)
void launch_pass_small(hipStream_t st, const DetectArgs& a, const TailArgs& t) {
  switch (a.sps) {
    case 2: hipLaunchKernelGGL((k_pass_small<1>), dim3(1), dim3(kThreads), 0, st, a, t); break;
    case 4: hipLaunchKernelGGL((k_pass_small<2>), dim3(1), dim3(kThreads), 0, st, a, t); break;
    case 8: hipLaunchKernelGGL((k_pass_small<4>), dim3(1), dim3(kThreads), 0, st, a, t); break;
    case 20: hipLaunchKernelGGL((k_pass_small<10>), dim3(1), dim3(kThreads), 0, st, a, t); break;
    default: hipLaunchKernelGGL((k_pass_small<0>), dim3(1), dim3(kThreads), 0, st, a, t); break;
  }
}
template <int MODE>
void launch_confidence(hipStream_t st, int grid, const DetectArgs& a, const Rec* out, const Summary* sum, int cap, float* ratio) {
  hipLaunchKernelGGL((k_confidence<MODE>), dim3(grid), dim3(kThreads), 0, st, a, out, sum, cap, ratio);
}

// opt-in Conservative FEC (ADSB_FLAG_FEC_CONSERVATIVE) of a pass's records, in place: one thread per list slot (step_grid),
// each leaves at once past sum->n_kept
void launch_fec(hipStream_t st, const Slot& s, Rec* out, const Summary* sum) {
  hipLaunchKernelGGL(k_fec, dim3(step_grid(s.tot, kThreads)), dim3(kThreads), 0, st, out, sum, (int)s.tot,
                     (Rec*)(s.host_cap > 0 ? s.h_out.p : nullptr), s.host_cap);
}

// whether the ordinary pass repairs: every pass of an ADSB_FLAG_FEC_SOFT context, and the fallback items of a batch call of an
// ADSB_FLAG_FEC_SOFT_BATCH one (batch_core)
inline bool soft_pass(const adsb_ctx* c) { return (c->flags & ADSB_FLAG_FEC_SOFT) != 0 || c->soft_fallback; }

// opt-in soft-decision repair (ADSB_FLAG_FEC_SOFT; adsb_softfec.hip) of a pass's records, in place behind launch_fec: one
// wavefront per record, the grid capped like k_confidence's, the bound sum->n_kept read on the device; one row per list slot
int launch_soft(adsb_ctx* c, hipStream_t st, const Slot& s, Rec* out, const Summary* sum) {
  const long long g = std::min<long long>((s.tot + kWaves - 1) / kWaves, (long long)c->n_cu * 8);
  const DetectArgs& a = s.args;
  const int e = adsb_softfec_host::launch_records(st, (unsigned)std::max(1ll, g), s.plan.mode, a.data, a.n, a.origin, a.scale, a.sps, &c->soft_rule,
                                                  out, &sum->n_kept, (int)s.tot, s.host_cap > 0 && out != (Rec*)s.h_out.p ? s.h_out.p : nullptr,
                                                  s.host_cap, s.d_soft.p);
  if (e) return fail(c, -EIO, "soft repair launch", (hipError_t)e);
  return 0;
}

// The library's key sort (adsb_device.h: k_dec_sort_*): stable, by the bits [lo_bit, hi_bit), four a pass -- a block histogram
// (hist: 16 words per tile of keys), one scan, a stable scatter, ping-pong between keys and sorted.  Both ranges in use give an
// odd number of passes (seven: the decode steps' address and "no key" marker; eleven: the store's keys): the result ends in sorted.
constexpr bool odd_passes(int lo_bit, int hi_bit) { return ((hi_bit - lo_bit + 3) / 4) % 2 == 1; }
static_assert(odd_passes(32, 60) && odd_passes(0, kFleetAddrBits + kFleetStreamBits), "the key sort's result has to end in sorted");
void launch_key_sort(hipStream_t st, unsigned long long* keys, unsigned long long* sorted, int n, int lo_bit, int hi_bit, unsigned* hist) {
  const int nblk = (n + kSortTile - 1) / kSortTile;
  for (int shift = lo_bit; shift < hi_bit; shift += 4) {
    hipLaunchKernelGGL(k_dec_sort_hist, dim3(nblk), dim3(kThreads), 0, st, (const unsigned long long*)keys, n, shift, hist);
    hipLaunchKernelGGL(k_dec_sort_scan, dim3(1), dim3(kThreads), 0, st, hist, nblk * 16);
    hipLaunchKernelGGL(k_dec_sort_scatter, dim3(nblk), dim3(kThreads), 0, st, (const unsigned long long*)keys, sorted, n, shift,
                       (const unsigned*)hist);
    std::swap(keys, sorted);
  }
}

// opt-in aircraft table (ADSB_FLAG_AIRCRAFT_TABLE): the table step of one published pass (list: out / mirror / sum; slices:
// bits14 / ok, n = ntags), in stream order behind every earlier pass's step: the three slots run on their own streams, so
// the step waits for the event recorded behind the previous one (pass n's verdict needs every announcement of passes < n)
// ADSB_FLAG_DECODE: the decode step of the same records, behind the last verdict (rows: cap rows; ts: the slices'
// timestamps, null for a pass's list).  The sort's buffers are the context's: every decode step waits for the one before.
int launch_dec(adsb_ctx* c, hipStream_t st, const AirArgs& a, unsigned g, DecRow* rows, const double* ts) {
  const size_t n = (size_t)a.cap;
  if (n == 0) return 0;
  const int nblk = (int)((n + kSortTile - 1) / kSortTile);
  const size_t tmp = (size_t)nblk * 16 * sizeof(unsigned);
  if (n * 8 > c->d_dec_keys.cap || n * 8 > c->d_dec_sorted.cap || tmp > c->d_dec_tmp.cap) {
    HIPCHK(c, hipEventSynchronize(c->air_ev));            // (the buffers may still be read by the step queued before)
    int r;
    if ((r = ensure(c, c->d_dec_keys, n * 8)) || (r = ensure(c, c->d_dec_sorted, n * 8)) || (r = ensure(c, c->d_dec_tmp, tmp))) return r;
  }
  DecArgs d{};
  d.air = a; d.ts = ts; d.start = c->dec_start; d.fs = c->fs; d.planes = c->d_planes; d.epoch = c->dec_epoch; d.all = c->dec_all;
  d.keys = (unsigned long long*)c->d_dec_keys.p; d.sorted = (const unsigned long long*)c->d_dec_sorted.p; d.rows = rows; d.seen = c->d_seen;
  hipLaunchKernelGGL(k_dec_classify, dim3(g), dim3(kThreads), 0, st, d);
  launch_key_sort(st, (unsigned long long*)c->d_dec_keys.p, (unsigned long long*)c->d_dec_sorted.p, (int)n, 32, 60, (unsigned*)c->d_dec_tmp.p);
  if (d.seen) hipLaunchKernelGGL(k_ages_fold, dim3(g), dim3(kThreads), 0, st, d);
  else hipLaunchKernelGGL(k_dec_fold, dim3(g), dim3(kThreads), 0, st, d);
  return 0;
}

int launch_air(adsb_ctx* c, hipStream_t st, AirArgs a, long long tot, DecRow* rows = nullptr, const double* ts = nullptr) {
  HIPCHK(c, hipStreamWaitEvent(st, c->air_ev, 0));
  const unsigned g = step_grid(tot, kThreads);
  a.table = c->d_air; a.st = c->d_air_st; a.fec = (c->flags & ADSB_FLAG_FEC_CONSERVATIVE) ? 1 : 0;
  hipLaunchKernelGGL(k_air_announce, dim3(g), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(k_air_verdict, dim3(g), dim3(kThreads), 0, st, a, 0);
  hipLaunchKernelGGL(k_air_cond, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_air_verdict, dim3(g), dim3(kThreads), 0, st, a, 1);
  if (c->flags & ADSB_FLAG_DECODE) { int r = launch_dec(c, st, a, g, rows, ts); if (r) return r; }
  HIPCHK(c, hipEventRecord(c->air_ev, st));
  return 0;
}

int launch_air_pass(adsb_ctx* c, Slot& s, hipStream_t st, Rec* out, int force = 0) {
  AirArgs a{};
  a.out = out; a.mirror = (out != (Rec*)s.h_out.p && s.host_cap > 0) ? (Rec*)s.h_out.p : nullptr;
  a.mirror_cap = a.mirror ? s.host_cap : 0;
  a.sum = &((Misc*)s.d_misc.p)->sum; a.cap = (int)s.tot; a.host_sum = s.h_sum; a.pass = s.air_pass; a.force = force;
  if (c->flags & ADSB_FLAG_DECODE) {
    int r = ensure_pinned(c, s.h_dec, (size_t)s.tot * sizeof(DecRow));
    if (r) return r;
  }
  return launch_air(c, st, a, s.tot, (DecRow*)s.h_dec.p, nullptr);
}

// the step state's `broken` word cleared behind every table step queued so far (before a pass that overflowed is re-run)
int air_unbreak(adsb_ctx* c, hipStream_t st) {
  HIPCHK(c, hipStreamWaitEvent(st, c->air_ev, 0));
  HIPCHK(c, hipMemsetAsync(&c->d_air_st->broken, 0, sizeof(int), st));
  HIPCHK(c, hipEventRecord(c->air_ev, st));
  return 0;
}

// an empty table (every key all ones) and a fresh step state, behind every table step queued so far; pass numbers restart
int air_clear(adsb_ctx* c) {
  if (c->air_next > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->air_ev, 0));
  HIPCHK(c, hipMemsetAsync(c->d_air, 0xFF, ((size_t)1 << 24) * sizeof(unsigned long long), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_air_st, 0, sizeof(AirState), c->stream));
  HIPCHK(c, hipEventRecord(c->air_ev, c->stream));
  c->air_next = 0;
  return 0;
}

// adsb_wait_for_event: the caller's pending events are waited for by `st`, the stream the next call's first operation runs on
int apply_ext(adsb_ctx* c, hipStream_t st) {
  for (int i = 0; i < c->n_ext; ++i) HIPCHK(c, hipStreamWaitEvent(st, c->ext_ev[i], 0));
  c->n_ext = 0;
  return 0;
}

// Everything after k_detect (and after k_longrun on the rare second pass): order, gate, compact, records.
int enqueue_tail(adsb_ctx* c, Slot& s) {
  const DetectArgs& a = s.args;
  const Plan& pl = s.plan;
  if (pl.air && !s.air_keep) s.air_pass = (c->air_next++) << 32;   // publication order = the order passes are queued in
  s.air_keep = false;
  Misc* misc = (Misc*)s.d_misc.p;
  hipStream_t ts = s.cs;
  if (s.direct) {
    ts = s.ds;
    // a small pass (few lists, at most kDirectRecs centres): the whole tail in one workgroup and one launch, on the
    // compute stream right behind its k_detect (nothing to overlap: the pass is a few microseconds of GPU time) -- or,
    // when k_detect itself is a single workgroup of |IQ|^2 float input (a GNU Radio work() call), the whole pass in ONE
    // launch (s.fused: k_detect was not launched)
    TailArgs t;
    t.cands = a.cands; t.recs = a.recs; t.blk_count = a.blk_count; t.blk_lastp = a.blk_lastp; t.blk_flags = a.blk_flags;
    t.blk_off = (int*)s.d_blk_off.p; t.nblk = s.nlists; t.rec_cap = s.rec_cap; t.long_count = a.long_count;
    t.long_lastp = a.long_lastp; t.sorted = (unsigned long long*)s.d_sorted.p; t.sorted_src = (unsigned*)s.d_sorted_src.p;
    t.seg_count = (int*)s.d_seg.p; t.sum = &misc->sum; t.host_sum = s.h_sum; t.out = (Rec*)s.h_out.p; t.out_cap = (int)s.tot;
    t.gate_on = pl.gate ? 1 : 0; t.head_n = pl.head_n; t.gate = 63ll * c->sps;
    t.gate_long = (long long)(pl.long_aware ? 119 : 63) * c->sps; t.prev_eob = pl.prev_eob_stream - pl.origin;
    s.seq = s.seq >= 0x7FFFFFF0 ? 1 : s.seq + 1;
    t.seq = s.seq;
    if (s.fused) launch_pass_small(ts, a, t);
    else ADSB_BY_MODE(pl.mode, launch_tail_small, ts, a, t);
    if ((c->flags & (ADSB_FLAG_FEC_CONSERVATIVE | ADSB_FLAG_AIRCRAFT_TABLE)) || soft_pass(c)) {
      // the repair / the table step follow the published pass number: the host waits for the event behind them instead
      // of polling
      if (c->flags & ADSB_FLAG_FEC_CONSERVATIVE) launch_fec(ts, s, (Rec*)s.h_out.p, &misc->sum);
      if (soft_pass(c)) { int r_ = launch_soft(c, ts, s, (Rec*)s.h_out.p, &misc->sum); if (r_) return r_; }
      if (pl.air) { int r_ = launch_air_pass(c, s, ts, (Rec*)s.h_out.p); if (r_) return r_; }
      HIPCHK(c, hipEventRecord(s.done, ts));
      return 0;
    }
    // the host polls the pass number in the pinned summary (finish): no completion event on the stream
    s.polled = true;
    return 0;
  }
  if (s.ds != s.cs) {
    // k_detect ran on a stream it shares with the k_detect launches of other passes: the tail, on its own stream, is ordered
    // after this pass's k_detect only -- the next k_detect can start while it runs.
    // With timing on, the event that closes k_detect's bracket doubles as the dependency.
    hipEvent_t dep = s.ev1_valid ? s.ev1 : s.det_done;
    if (!s.ev1_valid) HIPCHK(c, hipEventRecord(dep, s.ds));
    HIPCHK(c, hipStreamWaitEvent(s.cs, dep, 0));
  }
  // Every tail kernel is small enough to run on a CU BESIDE five resident k_detect workgroups (tests/test_abi.py holds
  // the limits).  Whether it should is a choice: beside the next pass's k_detect the tail finishes ~0.25 ms after its own
  // k_detect (results one pass earlier, two passes in flight suffice) but costs that k_detect 1-2 %; kept out -- k_order,
  // the first kernel of the chain, is launched with 8 KB of unused dynamic LDS, more than five k_detect workgroups leave
  // free on a CU -- it runs when that k_detect drains.  Throughput is the default, ADSB_FLAG_LOW_LATENCY selects the other.
  // (8 KB: measured.  A padding sized to what k_detect leaves free keeps the chain out more strictly and was SLOWER on
  // every workload: int16 791 vs 1039 Gsamples/s)
  const unsigned order_pad = (c->flags & ADSB_FLAG_LOW_LATENCY) ? 0u : 8192u;
  unsigned long long* sorted = (unsigned long long*)s.d_sorted.p;
  unsigned* sorted_src = (unsigned*)s.d_sorted_src.p;
  ADSB_BY_MODE(pl.mode, launch_order, ts, (s.nlists + kOrderLists - 1) / kOrderLists, order_pad, a, s.nlists, sorted, sorted_src,
               &misc->sum, &misc->acc);
  // k_resolve / k_count / k_compact work in segments of 256 list words; a workgroup past the last segment returns at once.
  // 2048 workgroups (eight per CU) give every segment of a headline pass (≈1900) its own workgroup: one round instead of
  // four (512 workgroups: k_compact 22 us, k_resolve 11, k_count 5 for 477 k centres)
  const int ag = 2048;
  unsigned fmask = 0u, fwant = 0u;
  if (pl.gate) {
    hipLaunchKernelGGL(k_resolve, dim3(ag), dim3(kThreads), 0, ts, sorted, (const Summary*)&misc->sum,
                       (long long)63 * c->sps, (long long)(pl.long_aware ? 119 : 63) * c->sps, pl.prev_eob_stream - pl.origin);
    fmask = kKept; fwant = kKept;
  }
  hipLaunchKernelGGL(k_count, dim3(ag), dim3(kThreads), 0, ts, (const unsigned long long*)sorted,
                     (const Summary*)&misc->sum, fmask, fwant, pl.head_n, (int*)s.d_seg.p);
  // k_compact's workgroup 0 stores the summary straight into s.h_sum (pinned host memory, device-visible): visible to the
  // host once the `done` event below has completed
  hipLaunchKernelGGL(k_compact, dim3(ag), dim3(kThreads), 0, ts, (const unsigned long long*)sorted, (const Rec*)a.recs, (const unsigned*)sorted_src,
                     &misc->sum, (const int*)s.d_seg.p, fmask, fwant, pl.head_n, (Rec*)(s.direct ? s.h_out.p : s.d_out.p), (int)s.tot,
                     a.long_count, a.long_lastp, &misc->acc, s.h_sum, (Rec*)(s.host_cap > 0 ? s.h_out.p : nullptr), s.host_cap);
  if (c->flags & ADSB_FLAG_FEC_CONSERVATIVE) launch_fec(ts, s, (Rec*)s.d_out.p, &misc->sum);
  if (soft_pass(c)) { int r_ = launch_soft(c, ts, s, (Rec*)s.d_out.p, &misc->sum); if (r_) return r_; }
  if (pl.air) { int r_ = launch_air_pass(c, s, ts, (Rec*)s.d_out.p); if (r_) return r_; }
  HIPCHK(c, hipEventRecord(s.done, ts));
  return 0;
}

// Queue the whole device pipeline of one plan on the compute stream; nothing here waits for the GPU.
int enqueue_pass(adsb_ctx* c, Slot& s, const Plan& pl, bool submitted) {
  HIPCHK(c, hipSetDevice(c->device));
  s.plan = pl;
  // the queue(s) of this pass (see adsb_ctx): a submitted pass on the slot's own stream; a blocking one alone on the
  // compute stream; a submitted pass on a caller-owned stream: k_detect there, the tail on the tail stream
  s.submitted = submitted;
  s.ds = s.cs = c->stream;
  if (submitted && c->split_tail) {
    if (!c->own_stream) {
      s.cs = c->tail_stream;                     // caller-owned compute stream: k_detect there, every tail on the tail stream
    } else {
      s.ds = s.cs = s.stream;
      // Three kinds of submitted passes keep their k_detect launches one behind the other on a stream of their own (the tail
      // follows on the slot's stream behind an event -- the arrangement of rounds 2-4):
      //  * timed ones (ADSB_FLAG_TIMING): the HIP events around k_detect are meant to bracket ONE launch that has the
      //    machine to itself -- two launches that overlap share the CUs and each reads twice as long;
      //  * passes over more than 4 GiB of input: a launch of over half a millisecond loses < 1 % in the hand-over to the next,
      //    and two HBM-bound launches that run side by side cost about that in DRAM locality (complex64, 2^30 samples:
      //    1.354-1.372 ms chained, 1.375-1.377 overlapped).  Everything smaller gains from the overlap: 2^28 samples +4-5 %,
      //    2^26 +20 %, 2^24 +38 %; the instruction-bound formats +2-6 % at any size (profiles/r05_ab_queue_arrangements.txt).
      //  * passes of the 8-bit formats over 1 GiB or more: their one-wavefront workgroups (adsb_device.h) leave no ragged
      //    end for the next launch to fill, and two instruction-bound launches side by side slow each other down (int8,
      //    2^30 samples: 0.568 ms in line, 0.607-0.617 overlapped; at 2^28 samples the same either way, below that the
      //    overlap wins by up to 20 %: profiles/r05_ab_8bit_workgroup_shape_and_schedule.txt).
      // No stream is added for that: the three slot streams take the three roles -- slot 0's every k_detect, slot 1's every
      // tail, slot 2's the record copies (finish) -- because the runtime multiplexes all streams of a process onto FOUR
      // hardware queues (GPU_MAX_HW_QUEUES), and a k_detect stream that shares its queue with a stream whose tail waits for
      // that k_detect stalls behind it: with a fourth stream for k_detect the timed 2^28-sample legs ran 10 % slower than
      // in round 4 (profiles/r05_pass_cost_timed_with_a_fourth_stream.txt).
      const long long in_bytes = (pl.scan_hi > 0 ? pl.scan_hi : 0) * (long long)mode_bytes(pl.mode);
      if ((c->flags & ADSB_FLAG_TIMING) || in_bytes > (4ll << 30) || (mode_is_iq8(pl.mode) && in_bytes >= (1ll << 30))) {
        s.ds = c->slot[0].stream;
        s.cs = c->slot[1].stream;
      }
    }
  }
  s.span = pl.scan_hi > 0 ? pl.scan_hi : 0;
  // A "unit" (one wavefront) walks one contiguous chunk and owns one output list.
  const int upb = det_waves(pl.mode);                      // units per k_detect workgroup: four, or one (8-bit formats)
  const int tile = kWTile;
  long long ntiles = (s.span + tile - 1) / tile;
  if (ntiles < 1) ntiles = 1;
  const int bpc = c->bpc[pl.mode];
  // chunks: one resident round of wavefronts is the floor, a bulk pass runs up to eight rounds of shorter ones (adsb_plan.h)
  long long units = 0, tiles_per = 0;
  plan_chunks(ntiles, (long long)c->n_cu * bpc * upb, &units, &tiles_per);
  const long long chunk = tiles_per * tile;
  // k_detect keeps pulse centres relative to the start of a unit's chunk in 32 bits
  if (chunk >= (1ll << 30)) return fail(c, -EINVAL, "input too long for one call on this device (chunk per wavefront >= 2^30 samples)");
  // a call of at most four units of |IQ|^2 floats may run as ONE launch of one four-wavefront workgroup (k_pass_small, below):
  // it gets four lists whatever it needs (units past `units` own nothing and report empty lists)
  const bool timing = (c->flags & ADSB_FLAG_TIMING) != 0;
  const bool can_fuse = units <= kWaves && pl.mode == ADSB_FMT_MAG2 && !timing;
  const int grid = can_fuse ? 1 : (int)((units + upb - 1) / upb);
  const int nlists = can_fuse ? kWaves : grid * upb;
  long long rc = (chunk / 256 + 64) << c->rec_cap_shift;
  if (rc > chunk / 2 + 8) rc = chunk / 2 + 8;   // there can never be more rises than that
  rc = (rc + 15) & ~15ll;                       // every list starts on a 128-byte line (k_detect's output stage writes whole lines)
  s.grid = grid; s.nlists = nlists; s.rec_cap = (int)rc; s.tot = (long long)nlists * rc; s.ntiles = ntiles; s.chunk = chunk;
  const long long long_cap = ntiles + 1;        // at most one long pulse per tile, plus the virtual rise
  int r;
  if ((r = ensure(c, s.d_cands, (size_t)s.tot * 8))) return r;
  if ((r = ensure(c, s.d_recs, (size_t)s.tot * sizeof(Rec)))) return r;
  if ((r = ensure(c, s.d_sorted, (size_t)s.tot * 8))) return r;
  if (s.tot >= (1ll << 32)) return fail(c, -EINVAL, "input too long for one call (list slots >= 2^32)");
  if ((r = ensure(c, s.d_sorted_src, (size_t)s.tot * sizeof(unsigned)))) return r;
  // A pass that can deliver only a few records (the GNU Radio work() calls: a few thousand samples) writes them from
  // k_compact straight into the pinned, device-visible result buffer: no device->host copy and no second
  // synchronisation at adsb_wait (the 48-byte summary travels the same way); bulk passes keep the DMA copy.
  const long long kDirectRecs = 16384;
  s.direct = s.tot <= kDirectRecs;
  // A MID-SIZE pass (up to 2^26 samples: tens of microseconds of k_detect, a few thousand records) gets both: k_compact
  // stores every record into d_out and the first kHostRecs of them ALSO straight into the pinned result buffer.  When the
  // pass delivers no more than that (the usual case) adsb_wait returns as soon as the tail's event has completed -- no
  // device->host copy and no second synchronisation (~12 us of a pass whose host side costs 40, tools/pass_cost.py); when
  // it delivers more, the copy runs as for a bulk pass (d_out is always complete).  Bulk passes are left alone: their
  // records are megabytes, the DMA engine moves them beside the next pass's kernels.
  const long long kMidTiles = 65536, kHostRecs = 32768;
  s.host_cap = 0;
  if (s.direct) { if ((r = ensure_pinned(c, s.h_out, (size_t)s.tot * sizeof(Rec), true))) return r; }
  else {
    if ((r = ensure(c, s.d_out, (size_t)s.tot * sizeof(Rec)))) return r;
    if (ntiles <= kMidTiles) {
      if ((r = ensure_pinned(c, s.h_out, (size_t)kHostRecs * sizeof(Rec), true))) return r;
      s.host_cap = (int)kHostRecs;
    }
  }
  if (soft_pass(c) && (r = ensure(c, s.d_soft, (size_t)s.tot * sizeof(adsb_soft_fix)))) return r;
  if ((r = ensure(c, s.d_seg, (size_t)(s.tot / kThreads + 2) * sizeof(int)))) return r;
  if ((r = ensure(c, s.d_blk_count, (size_t)nlists * sizeof(int)))) return r;
  if ((r = ensure(c, s.d_blk_lastp, (size_t)nlists * sizeof(long long)))) return r;
  if ((r = ensure(c, s.d_blk_flags, (size_t)nlists * sizeof(unsigned)))) return r;
  if ((r = ensure(c, s.d_blk_off, (size_t)nlists * sizeof(int)))) return r;
  if ((r = ensure(c, s.d_long, (size_t)long_cap * sizeof(LongRise)))) return r;
  if (!s.d_misc.p) {
    if ((r = ensure(c, s.d_misc, sizeof(Misc)))) return r;
    // on the compute stream (the context's streams are non-blocking: a legacy-stream memset would not be ordered
    // before the first k_detect); afterwards k_compact re-zeroes the list head every pass
    HIPCHK(c, hipMemsetAsync(s.d_misc.p, 0, sizeof(Misc), s.ds));
  }
  Misc* misc = (Misc*)s.d_misc.p;

  DetectArgs& a = s.args;
  a.data = pl.d_data; a.n = pl.n; a.in0_base = pl.in0_base; a.scan_lo = pl.scan_lo; a.scan_hi = pl.scan_hi;
  a.fall_hi = pl.fall_hi; a.dem_hi = pl.dem_hi; a.origin = pl.origin; a.chunk = chunk; a.thr = c->thr;
  a.prev_in0 = pl.prev_in0; a.scale = c->scale[pl.mode]; a.sps = c->sps; a.end_is_call_end = pl.end_is_call_end; a.rec_cap = s.rec_cap;
  a.long_aware = pl.long_aware ? 1 : 0;
  a.long_cap = (int)long_cap; a.cands = (unsigned long long*)s.d_cands.p; a.recs = (Rec*)s.d_recs.p; a.blk_count = (int*)s.d_blk_count.p;
  a.blk_lastp = (long long*)s.d_blk_lastp.p; a.blk_flags = (unsigned*)s.d_blk_flags.p;
  a.longlist = (LongRise*)s.d_long.p; a.long_count = &misc->long_count; a.long_lastp = &misc->long_lastp;

  s.fused = s.direct && can_fuse;
  // what this pass's first kernel has to wait for: its own upload (host-fed submission), the caller's events (adsb_wait_for_event)
  if (s.h2d_pending) { HIPCHK(c, hipStreamWaitEvent(s.ds, s.h2d_done, 0)); s.h2d_pending = false; }
  { int r_ = apply_ext(c, s.ds); if (r_) return r_; }
  if (!s.fused) {
    if (timing) HIPCHK(c, hipEventRecord(s.ev0, s.ds));
    ADSB_BY_MODE(pl.mode, launch_detect, c, s.ds, a, grid);
    if (timing) HIPCHK(c, hipEventRecord(s.ev1, s.ds));
  }
  c->stats.detect_grid = (uint64_t)grid; c->stats.blocks_per_cu = (uint64_t)c->bpc[pl.mode];
  c->stats.calls++;
  s.busy = true;
  s.ev1_valid = timing;
  s.polled = false;
  return enqueue_tail(c, s);
}
// ... and a pass that could not be queued leaves its slot free: no caller has a ticket to release
int enqueue(adsb_ctx* c, Slot& s, const Plan& pl, bool submitted) {
  const int r = enqueue_pass(c, s, pl, submitted);
  if (r) s.busy = false;
  return r;
}

// The pass's lists overflowed: the capacity multiplier grows and the pass is queued again (one call: not counted twice).
int requeue_grown(adsb_ctx* c, Slot& s) {
  if ((long long)s.rec_cap >= s.chunk / 2 + 8) return fail(c, -EIO, "centre list overflow at maximum size");
  c->rec_cap_shift++;
  c->stats.retries++;
  const int r = enqueue(c, s, s.plan, s.submitted);
  if (r) return r;
  c->stats.calls--;
  return 0;
}

// Wait for a queued call; handle the two rare outcomes that need a second pass (pulses longer than the
// LDS window; per-workgroup list overflow); bring the records to pinned host memory.
// ADSB_FLAG_AIRCRAFT_TABLE after a centre-list overflow: the overflowed pass skipped its table step and set `broken`, so
// every step queued behind it skipped too (kAirSkipped in its summary).  Every pass in flight is settled, in publication
// order: an overflowed one is re-run under its own number (behind a cleared `broken`), a skipped step is re-run.  Nothing
// is submitted meanwhile, so each verdict again sees exactly the announcements of the passes before it.
int air_settle_all(adsb_ctx* c) {
  Slot* order[ADSB_MAX_IN_FLIGHT];
  int n = 0;
  for (Slot& sl : c->slot)
    if (sl.busy && sl.plan.air) {
      int k = n++;
      for (; k > 0 && order[k - 1]->air_pass > sl.air_pass; --k) order[k] = order[k - 1];
      order[k] = &sl;
    }
  for (int i = 0; i < n; ++i) {
    Slot& s = *order[i];
    for (int attempt = 0;; ++attempt) {
      if (attempt == 16) return fail(c, -EIO, "centre list capacity did not converge");
      HIPCHK(c, hipEventSynchronize(s.done));
      HIPCHK(c, hipGetLastError());
      const hipStream_t ts = s.direct ? s.ds : s.cs;
      int r;
      if (s.h_sum->overflow) {
        if ((r = air_unbreak(c, ts))) return r;
        s.air_keep = true;
        if ((r = requeue_grown(c, s))) return r;
        continue;
      }
      if (s.h_sum->flags & kAirSkipped) {
        s.h_sum->flags &= ~kAirSkipped;
        if ((r = launch_air_pass(c, s, ts, (Rec*)(s.direct ? s.h_out.p : s.d_out.p), 1))) return r;
        HIPCHK(c, hipEventRecord(s.done, ts));
        continue;
      }
      break;
    }
  }
  return 0;
}

int finish_pass(adsb_ctx* c, Slot& s, Summary* sum, int32_t* n_res) {
  HIPCHK(c, hipSetDevice(c->device));
  const bool timing = (c->flags & ADSB_FLAG_TIMING) != 0;
  for (int attempt = 0; attempt < 16; ++attempt) {
    if (s.polled) {
      // a one-workgroup pass: its last store is the pass number (publish_small); spin on it -- bounded: a kernel that died
      // never stores it, and the stream synchronisation below reports why
      // The spin is SHORT (the pass itself takes ~10 us; ~50 us covers a pass queued behind one or two others): a pass that
      // sits behind more work than that -- a caller-owned stream, several submissions in flight -- is waited for by
      // blocking on the stream instead of burning the calling thread's core (in GNU Radio: the framer's work() thread).
      const volatile int* seqp = &s.h_sum->pad_;
      const auto t0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (*seqp != s.seq) {
        cpu_relax();
        if ((++spins & 0x3Fu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(50)) break;
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (*seqp != s.seq) {
        HIPCHK(c, hipStreamSynchronize(s.ds));
        HIPCHK(c, hipGetLastError());
        std::atomic_thread_fence(std::memory_order_acquire);
        if (*seqp != s.seq) return fail(c, -EIO, "small pass finished without publishing its summary");
        c->stats.poll_fallbacks++;
      }
    } else {
      HIPCHK(c, hipEventSynchronize(s.done));
      HIPCHK(c, hipGetLastError());
      if (s.plan.air && (s.h_sum->overflow || (s.h_sum->flags & kAirSkipped))) {
        int r_ = air_settle_all(c);
        if (r_) return r_;
      }
    }
    if (timing) {
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, s.ev0, s.ev1));
      c->stats.detect_launches++;
      c->stats.detect_ms += ms;
      if (c->det_hist.size() < (size_t)adsb_ctx::kHist) c->det_hist.resize(adsb_ctx::kHist);
      c->det_hist[c->det_hist_n++ % adsb_ctx::kHist] = ms;
      // idle time on the compute stream between the previous pass's k_detect and this one (pipelined use)
      // idle time on the compute stream between this pass's k_detect and the NEXT pass's (already queued in
      // pipelined use; its events are valid if that pass has been collected or is complete -- best effort)
      const int me = (int)(&s - c->slot);
      Slot& nxt = c->slot[(me + 1) % ADSB_MAX_IN_FLIGHT];
      if (nxt.busy && nxt.ev1_valid) {
        float gap = 0;
        if (hipEventElapsedTime(&gap, s.ev1, nxt.ev0) == hipSuccess && gap >= 0 && gap < 100.0f) {
          c->stats.detect_gap_ms += gap; c->stats.detect_gaps++;
        } else (void)hipGetLastError();
      }
      c->stats.detect_samples += (uint64_t)s.span;
      c->stats.detect_bytes += (uint64_t)s.span * (uint64_t)mode_bytes(s.plan.mode);
    }
    if (s.h_sum->overflow) {
      int r = requeue_grown(c, s);
      if (r) return r;
      continue;
    }
    if (s.h_sum->long_count > 0) { c->stats.longrun_calls++; c->stats.longrun_pulses += (uint64_t)s.h_sum->long_count; }
    if (s.h_sum->long_count > s.args.long_cap) return fail(c, -EIO, "long-rise list overflow");
    *sum = *s.h_sum;
    const int nres = sum->n_kept;
    // the records are already in h_out: a one-workgroup pass (all of them), or a mid-size pass that delivered no more than
    // k_compact stored there beside d_out (enqueue)
    const bool in_host = (s.direct || nres <= s.host_cap) && s.h_out.p != nullptr;
    int r = in_host ? 0 : ensure_pinned(c, s.h_out, (size_t)(nres > 0 ? nres : 1) * sizeof(Rec), true);
    if (r) return r;
    const Rec* recs_dev = (const Rec*)(s.direct ? s.h_out.p : s.d_out.p);
    if (nres > 0 && (!in_host || (c->flags & ADSB_FLAG_CONFIDENCE) || soft_pass(c))) {
      // on the pass's own stream (idle: its last kernel has completed); never on a caller-owned one
      // (a submitted pass that shares its stream with the passes behind it -- kernels in line, or ADSB_FLAG_SINGLE_STREAM --
      // copies on the context's record-copy stream: on its own one the copy would wait for everything queued since)
      // Slot 2's stream is free for that in a context whose passes are all in line (timed contexts; bulk 8-bit / > 4 GiB
      // streams) -- and it keeps the context at three busy streams, one hardware queue each (a fourth busy stream shares a
      // queue with one of the three and serialises behind it: the 8-bit legs ran 6 % slower with a copy stream of their own,
      // profiles/r06_ab_record_copy_stream.txt).  Only when slot 2 itself holds an overlapped pass (a context that mixes in-line
      // and overlapped passes) would the copy of an older pass wait for that younger one: then a copy stream of its own.
      const bool shared = s.ds != s.cs || (s.submitted && !c->split_tail);
      const Slot& s2 = c->slot[2];
      const bool slot2_taken = &s2 != &s && s2.busy && s2.ds == s2.stream;
      if (c->own_stream && shared && slot2_taken && !c->d2h_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->d2h_stream.p, hipStreamNonBlocking));
      const hipStream_t xs = !c->own_stream ? c->copy_stream.p : (shared ? (slot2_taken ? c->d2h_stream.p : c->slot[2].stream.p) : s.cs);
      if (!in_host)
        HIPCHK(c, hipMemcpyAsync(s.h_out.p, s.d_out.p, (size_t)nres * sizeof(Rec), hipMemcpyDeviceToHost, xs));
      if (c->flags & ADSB_FLAG_CONFIDENCE) {
        // opt-in (demod.py:97-101): bit1/bit0 ratios of the delivered records, computed now that their number is
        // known -- one more small kernel and copy on the copy stream, paid only by callers who ask for it
        const size_t rb = (size_t)nres * 112 * sizeof(float);
        if ((r = ensure(c, s.d_ratio, rb)) || (r = ensure_pinned(c, s.h_ratio, rb))) return r;
        HIPCHK(c, hipMemsetAsync(s.d_ratio.p, 0, rb, xs));
        int cg = (nres + kWaves - 1) / kWaves;
        if (cg > c->n_cu * 8) cg = c->n_cu * 8;
        ADSB_BY_MODE(s.plan.mode, launch_confidence, xs, cg, s.args, recs_dev,
                     (const Summary*)&((Misc*)s.d_misc.p)->sum, nres, (float*)s.d_ratio.p);
        HIPCHK(c, hipMemcpyAsync(s.h_ratio.p, s.d_ratio.p, rb, hipMemcpyDeviceToHost, xs));
      }
      if (soft_pass(c)) {
        // the records' adsb_soft_fix rows travel with them (adsb_last_soft)
        if ((r = ensure_pinned(c, s.h_soft, (size_t)nres * sizeof(adsb_soft_fix)))) return r;
        HIPCHK(c, hipMemcpyAsync(s.h_soft.p, s.d_soft.p, (size_t)nres * sizeof(adsb_soft_fix), hipMemcpyDeviceToHost, xs));
      }
      HIPCHK(c, hipStreamSynchronize(xs));
      HIPCHK(c, hipGetLastError());
    }
    if (c->flags & ADSB_FLAG_FEC_SOFT) c->soft_dm = nullptr;
    s.nres = nres;
    *n_res = nres;
    return 0;
  }
  return fail(c, -EIO, "centre list capacity did not converge");
}
// ... and the slot is free afterwards, whatever came of the call: a failed call must not leave its ticket busy for good
int finish(adsb_ctx* c, Slot& s, Summary* sum, int32_t* n_res) {
  const int r = finish_pass(c, s, sum, n_res);
  s.busy = false;
  return r;
}

// Synchronous form used by every blocking entry point.
int run_pipeline(adsb_ctx* c, const Plan& pl, Summary* sum, int32_t* n_res) {
  int r = require_idle(c, kCallPending);
  if (r) return r;
  Slot& s = c->slot[0];
  c->last_slot = 0;
  if ((r = enqueue(c, s, pl, false))) return r;
  return finish(c, s, sum, n_res);
}

int deliver(adsb_ctx* c, int32_t nres, adsb_burst* out, int32_t cap, int32_t* n_out) {
  if (n_out) *n_out = nres;
  if (out) {
    if (nres > cap) return fail(c, -ENOSPC, "output array too small");
    if (nres > 0) memcpy(out, c->slot[c->last_slot].h_out.p, (size_t)nres * sizeof(adsb_burst));
  }
  return 0;
}

int canonical(adsb_ctx* c, int mode, const void* d_data, int64_t n, int64_t abs_offset, adsb_burst* out,
              int32_t cap, int32_t* n_out) {
  if (!c || n < 0) return -EINVAL;
  if (((uintptr_t)d_data & 15u) != 0) return fail(c, -EINVAL, "device pointer must be 16-byte aligned");
  Plan pl = plan_canonical(mode, d_data, n, abs_offset, c->sps);
  pl.long_aware = (c->flags & ADSB_FLAG_LONG_AWARE_GATE) != 0;
  pl.air = (c->flags & ADSB_FLAG_AIRCRAFT_TABLE) != 0;
  Summary s;
  int32_t nres = 0;
  if (n == 0) { c->slot[c->last_slot].nres = 0; if (n_out) *n_out = 0; return 0; }
  int rc = run_pipeline(c, pl, &s, &nres);
  if (rc) return rc;
  return deliver(c, nres, out, cap, n_out);
}

bool is_pinned_host(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // pageable
  return at.type == hipMemoryTypeHost;
}

// The address under which the DEVICE sees a page-locked host buffer.  For hipHostMalloc'ed memory it equals the host
// address on ROCm; for memory page-locked in place (adsb_host_register -> hipHostRegister) HIP only promises access
// through the alias hipHostGetDevicePointer returns.  nullptr: not mapped -- the caller stages instead.
const void* device_alias(const void* host) {
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, const_cast<void*>(host), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return dev;
}

int ensure_pool(adsb_ctx* c) {
  if (c->pool) return 0;
  c->pool.reset(new (std::nothrow) CopyPool());
  if (!c->pool) return fail(c, -ENOMEM, "copy pool");
  const unsigned hw = std::thread::hardware_concurrency();
  const int nt = c->copy_threads >= 0 ? c->copy_threads : (hw >= 16 ? 5 : (hw >= 4 ? 2 : 0));     // workers besides the caller
  if (c->have_local_cpus && !(c->flags & ADSB_FLAG_NO_NUMA_BINDING)) {
    // the GPU's local cpus, but never outside the mask the PROCESS was given (taskset, numactl --physcpubind, a cgroup):
    // the workers run on the intersection, or stay unbound when that is empty
    cpu_set_t mine, both;
    CPU_ZERO(&mine);
    if (sched_getaffinity(0, sizeof(mine), &mine) == 0) {
      CPU_AND(&both, &mine, &c->local_cpus);
      if (CPU_COUNT(&both) > 0) { c->pool->cpus = both; c->pool->have_cpus = true; }
    }
  }
  c->pool->start(nt);
  return 0;
}

// Pageable host memory -> device memory on `stream` through the ring of pinned chunks: the host copy of chunk k+1 (split
// over the context's copy threads) runs beside the DMA of chunk k.  Returns once the last DMA is QUEUED.
int staged_copy(adsb_ctx* c, void* d_dst, const void* host, size_t bytes, hipStream_t stream) {
  constexpr size_t kRingChunk = (size_t)16 << 20;
  for (PinnedPtr<void>& r : c->h_ring)
    if (!r) HIPCHK(c, host_alloc_near(c, &r.p, kRingChunk));    // the staging ring: on the GPU's NUMA node
  int rc = ensure_pool(c);
  if (rc) return rc;
  // the host copy of piece k+1 runs beside the DMA of piece k: a source of a few megabytes (a GNU Radio work() call of a
  // megasample) is cut into at least four pieces, a bulk one into whole 16 MiB ring chunks
  size_t kChunk = kRingChunk;
  while (kChunk > ((size_t)1 << 20) && bytes < 4 * kChunk) kChunk >>= 1;
  for (size_t off = 0; off < bytes; off += kChunk) {
    const size_t m = bytes - off < kChunk ? bytes - off : kChunk;
    const int b = (int)(c->ring_k++ % (unsigned)adsb_ctx::kRing);
    if (c->ring_used[b]) HIPCHK(c, hipEventSynchronize(c->ring_done[b]));      // the chunk's previous DMA has read it
    c->pool->copy((char*)c->h_ring[b].p, (const char*)host + off, m);
    HIPCHK(c, hipMemcpyAsync((char*)d_dst + off, c->h_ring[b], m, hipMemcpyHostToDevice, stream));
    HIPCHK(c, hipEventRecord(c->ring_done[b], stream));
    c->ring_used[b] = true;
  }
  return 0;
}

// Host buffer -> something the kernels can read, for the blocking entry points (the buffer only has to stay valid until
// the call returns).  Large inputs are copied to the device: page-locked sources (adsb_host_alloc, hipHostMalloc, torch
// pin_memory) go straight over PCIe, pageable ones through the context's pinned staging buffer.  Small inputs (the GNU
// Radio work() calls: a few thousand samples) are not copied to the device at all: the kernels read the page-locked
// copy in place over PCIe, once -- one operation fewer in a call whose cost is operations, not bytes.
int upload(adsb_ctx* c, const void* host, size_t bytes, void** d_out) {
  const size_t kZeroCopyBytes = (size_t)256 << 10;
  int rc;
  if ((rc = apply_ext(c, c->stream))) return rc;
  const void* src = host;
  const bool pinned = is_pinned_host(host);
  const bool small = bytes <= kZeroCopyBytes;
  const void* alias = (pinned && small) ? device_alias(host) : nullptr;     // only the in-place path needs it
  if (!small && !pinned && bytes >= ((size_t)4 << 20)) {
    // multi-megabyte pageable input (a GNU Radio block run with large chunks): chunked through the pinned ring
    if ((rc = ensure(c, c->d_in, bytes + 64))) return rc;
    if ((rc = staged_copy(c, c->d_in.p, host, bytes, c->stream))) return rc;
    *d_out = c->d_in.p;
    return 0;
  }
  if (!pinned || (small && (!alias || ((uintptr_t)alias & 15u) != 0))) {
    if ((rc = ensure_pinned(c, c->h_stage, bytes))) return rc;
    memcpy(c->h_stage.p, host, bytes);
    src = c->h_stage.p;
    alias = c->h_stage.p;                                   // hipHostMalloc'ed: one address on both sides
  }
  if (small) {
    *d_out = const_cast<void*>(alias);
    return 0;
  }
  if ((rc = ensure(c, c->d_in, bytes + 64))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_in.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  *d_out = c->d_in.p;
  return 0;
}

// ---- adsb_process_batch*: many independent streams, one workgroup each (k_batch), one dense result (k_batch_pack) ----------
// k_batch is instantiated per input format for 2 Msps (the rate of the receivers that come in fleets: RTL-SDR, HackRF) and
// with the run-time tap stride for every other rate: ten instances, not twenty-five -- each is a detect_body plus a tail, and
// the library's build time is its kernels'.  The 8-bit formats run the generic-scale conversion whatever the scale is (the
// power-of-two instances of k_detect are bit-identical to it: tests/test_conversion_exact.py).
template <int MODE>
void launch_batch(hipStream_t st, int sps, int n_items, const DetectArgs* da, const TailArgs* ta, int* kept) {
  if (sps == 2) hipLaunchKernelGGL((k_batch<MODE, 1>), dim3(n_items), dim3(kThreads), 0, st, da, ta, kept);
  else hipLaunchKernelGGL((k_batch<MODE, 0>), dim3(n_items), dim3(kThreads), 0, st, da, ta, kept);
}

int check_batch(adsb_ctx* c, int fmt, const adsb_batch_item* items, int32_t n_items, adsb_burst* out, int32_t cap,
                int32_t* item_first, int32_t* n_out) {
  if (!c) return -EINVAL;
  if (fmt < 0 || fmt >= ADSB_FMT_COUNT) return fail(c, -EINVAL, "adsb_process_batch: bad format");
  if (n_items < 0 || (n_items > 0 && !items) || cap < 0 || (cap > 0 && !out) || !item_first || !n_out)
    return fail(c, -EINVAL, "adsb_process_batch: bad argument");
  if (c->flags & (ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE | ADSB_FLAG_CONFIDENCE))
    return fail(c, -EINVAL, "adsb_process_batch: not for ADSB_FLAG_AIRCRAFT_TABLE / _DECODE / _CONFIDENCE contexts (one receiver each)");
  if (c->flags & ADSB_FLAG_FEC_SOFT) return fail(c, -EINVAL, "adsb_process_batch: not for ADSB_FLAG_FEC_SOFT contexts");
  for (int32_t i = 0; i < n_items; ++i) {
    if (items[i].reserved != 0u) return fail(c, -EINVAL, "adsb_process_batch: item.reserved must be 0");
    if (items[i].n < 0) return fail(c, -EINVAL, "adsb_process_batch: item.n < 0");
    if (items[i].n > 0 && !items[i].data) return fail(c, -EINVAL, "adsb_process_batch: item.data is NULL");
    if (((uintptr_t)items[i].data & 15u) != 0) return fail(c, -EINVAL, "adsb_process_batch: item.data must be 16-byte aligned");
  }
  return require_idle(c, kCallPending);
}

// the dense list and item_first are 32-bit: a batch whose lists have 2^31 slots or more is refused
int batch_slots_ok(adsb_ctx* c, const adsb_batch_item* items, int32_t n_items) {
  long long slots = 0;
  for (int32_t i = 0; i < n_items; ++i)
    if (items[i].n > 0 && items[i].n <= kBatchItemMax) slots += (long long)kWaves * plan_batch_item(items[i].n, c->sps, kWaves, kWTile).rec_cap;
  if (slots >= (1ll << 31)) return fail(c, -EINVAL, "adsb_process_batch: batch too large for one call (list slots >= 2^31)");
  return 0;
}

// One item of a batch pass as batch_core runs it: its plan (the buffer the device reads included), its threshold, and who
// runs it -- k_batch, nobody (no samples, or nothing owned), or the host through the ordinary pass (longer than
// ADSB_BATCH_ITEM_MAX; k_batch hands back the items whose lists overflow itself).
struct BatchWork { Plan plan; float thr; enum Kind { kEmpty, kKernel, kHost } kind; };
// the two small kernels of a stream batch around k_batch / the pack step (run_stream_batch), their tables on the device
struct StreamHooks { const StreamStage* stage; const StreamSave* save; StreamStatus* status; };
// What batch_core leaves: the dense list of the items k_batch finished (item i: packed[first[i] .. first[i + 1]), kept[i]
// >= 0) and, per item it did not (kept[i] < 0), the records and the Summary flags of its ordinary pass (fb[fb_of[i]]).
struct BatchResult {
  const adsb_burst* packed = nullptr;
  const int* first = nullptr;
  const int* kept = nullptr;
  long long nb = 0;
  int32_t nfb = 0;
  std::vector<std::vector<adsb_burst>> fb;
  std::vector<unsigned> fb_flags;
  std::vector<int32_t> fb_of;
  // ADSB_FLAG_FEC_SOFT_BATCH: rows[t] belongs to packed[t], fb_rows[k][t] to fb[k][t]
  const adsb_soft_fix* rows = nullptr;
  std::vector<std::vector<adsb_soft_fix>> fb_rows;
};

// The device pass of a batch: the tables, k_batch, k_batch_pack, k_fec, and the ordinary pass for what is left.
int batch_core(adsb_ctx* c, int fmt, const std::vector<BatchWork>& work, const StreamHooks* hooks, BatchResult* R) {
  const int32_t n_items = (int32_t)work.size();
  BatchBufs& B = c->bt;
  const hipStream_t st = c->stream;
  int r;
  // Scratch PER ITEM, laid out one item after the other (adsb_plan.h: plan_batch_layout)
  std::vector<BatchLay> lay((size_t)n_items);
  size_t total = 0;
  long long packed_cap = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    BatchLay& L = lay[(size_t)i];
    L.slots = 0;
    if (work[(size_t)i].kind != BatchWork::kKernel) continue;
    // (plan_batch_item takes a canonical call's length: its scan range ends 8 * sps - 1 samples in front of that)
    L = plan_batch_layout(total, plan_batch_item(work[(size_t)i].plan.scan_hi + (8ll * c->sps - 1), c->sps, kWaves, kWTile), kWaves,
                          kThreads, sizeof(Rec), sizeof(LongRise));
    total = L.end;
    packed_cap += L.slots;
  }
  // the dense list and item_first are 32-bit: a batch whose lists have 2^31 slots or more is refused
  if (packed_cap >= (1ll << 31)) return fail(c, -EINVAL, "adsb_process_batch: batch too large for one call (list slots >= 2^31)");
  const long long kHostRecs = 32768;
  // ADSB_FLAG_FEC_SOFT_BATCH: the soft repair's own item table behind the two argument tables
  const bool soft = (c->flags & ADSB_FLAG_FEC_SOFT_BATCH) != 0;
  typedef adsb_softfec_batch_host::Item SoftItem;
  static_assert((sizeof(DetectArgs) + sizeof(TailArgs)) % alignof(SoftItem) == 0, "the soft repair's table is aligned behind the others");
  const size_t soft_tab = (size_t)n_items * (sizeof(DetectArgs) + sizeof(TailArgs));
  const size_t tab_bytes = soft_tab + (soft ? (size_t)n_items * sizeof(SoftItem) : 0);
  if (soft && ((r = ensure(c, B.d_soft_items, (size_t)n_items * sizeof(SoftItem))) ||
               (r = ensure(c, B.d_soft_rows, (size_t)(packed_cap + 1) * sizeof(adsb_soft_fix)))))
    return r;
  if ((r = ensure(c, B.d_scratch, total + 128))) return r;
  if ((r = ensure(c, B.d_fixed, (size_t)n_items * sizeof(BatchFixed)))) return r;
  if ((r = ensure(c, B.d_da, (size_t)n_items * sizeof(DetectArgs)))) return r;
  if ((r = ensure(c, B.d_ta, (size_t)n_items * sizeof(TailArgs)))) return r;
  if ((r = ensure(c, B.d_kept, (size_t)n_items * sizeof(int)))) return r;
  if ((r = ensure(c, B.d_packed, (size_t)(packed_cap + 1) * sizeof(Rec)))) return r;
  if ((r = ensure(c, B.d_tot, sizeof(Summary)))) return r;
  if ((r = ensure_pinned(c, B.h_tab, tab_bytes))) return r;
  if ((r = ensure_pinned(c, B.h_first, (size_t)(2 * (size_t)n_items + 1) * sizeof(int), true))) return r;
  if ((r = ensure_pinned(c, B.h_out, (size_t)kHostRecs * sizeof(Rec), true))) return r;
  long long host_cap = (long long)(B.h_out.cap / sizeof(Rec));
  if (host_cap > kHostRecs) host_cap = kHostRecs;

  DetectArgs* hda = (DetectArgs*)B.h_tab.p;
  TailArgs* hta = (TailArgs*)((char*)B.h_tab.p + (size_t)n_items * sizeof(DetectArgs));
  memset(B.h_tab.p, 0, tab_bytes);
  char* const sc = (char*)B.d_scratch.p;
  BatchFixed* const fx = (BatchFixed*)B.d_fixed.p;
  const bool long_aware = (c->flags & ADSB_FLAG_LONG_AWARE_GATE) != 0;
  for (int32_t i = 0; i < n_items; ++i) {
    const BatchLay& L = lay[(size_t)i];
    const BatchWork& w = work[(size_t)i];
    if (L.slots == 0) { hda[i].n = w.kind == BatchWork::kEmpty ? 0 : -1; continue; }     // empty, or the host's own (too long)
    fill_batch_item(hda[i], hta[i], w.plan, L, sc, fx[i], w.thr, c->scale[fmt], c->sps, long_aware, kWaves);
    // the samples as the item's k_batch workgroup reads them; the other items' ranges in the dense list are empty
    if (soft) ((SoftItem*)((char*)B.h_tab.p + soft_tab))[i] = SoftItem{w.plan.d_data, w.plan.n, w.plan.origin, 0};
  }
  if ((r = apply_ext(c, st))) return r;
  if (soft) HIPCHK(c, hipMemcpyAsync(B.d_soft_items.p, (char*)B.h_tab.p + soft_tab, (size_t)n_items * sizeof(SoftItem), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(B.d_da.p, hda, (size_t)n_items * sizeof(DetectArgs), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(B.d_ta.p, hta, (size_t)n_items * sizeof(TailArgs), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(B.d_fixed.p, 0, (size_t)n_items * sizeof(BatchFixed), st));
  int* const h_first = (int*)B.h_first.p;
  int* const h_kept = h_first + n_items + 1;
  if (hooks) hipLaunchKernelGGL(k_stream_stage, dim3(n_items), dim3(kThreads), 0, st, hooks->stage);
  ADSB_BY_MODE(fmt, launch_batch, st, c->sps, (int)n_items, (const DetectArgs*)B.d_da.p, (const TailArgs*)B.d_ta.p, (int*)B.d_kept.p);
  hipLaunchKernelGGL(k_batch_pack, dim3(n_items), dim3(kThreads), 0, st, (const TailArgs*)B.d_ta.p, (const int*)B.d_kept.p,
                     (int)n_items, (Rec*)B.d_packed.p, (int)packed_cap, h_first, h_kept, (Summary*)B.d_tot.p, (Rec*)B.h_out.p,
                     (int)host_cap);
  if (c->flags & ADSB_FLAG_FEC_CONSERVATIVE) {
    hipLaunchKernelGGL(k_fec, dim3(step_grid(packed_cap, kThreads)), dim3(kThreads), 0, st, (Rec*)B.d_packed.p,
                       (const Summary*)B.d_tot.p, (int)packed_cap, (Rec*)B.h_out.p, (int)host_cap);
  }
  if (soft) {
    // behind k_fec, on the packed list: item i's records against item i's samples (a stream item's: its staging buffer, which
    // k_stream_save below only reads), first[] as k_batch_pack has just written it
    const int e = adsb_softfec_batch_host::launch_items(st, (int)n_items, fmt, B.d_soft_items.p, h_first, c->scale[fmt], c->sps, &c->soft_rule,
                                                        B.d_packed.p, (int)packed_cap, B.h_out.p, (int)host_cap, B.d_soft_rows.p);
    if (e) { (void)hipStreamSynchronize(st); return fail(c, -EIO, "soft repair launch", (hipError_t)e); }
  }
  if (hooks) {
    hipLaunchKernelGGL(k_stream_save, dim3(n_items), dim3(kThreads), 0, st, hooks->save, (const TailArgs*)B.d_ta.p,
                       (const int*)B.d_kept.p, hooks->status);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));
  std::atomic_thread_fence(std::memory_order_acquire);
  c->stats.calls++;
  const long long nb = h_first[n_items];
  if (nb < 0 || nb > packed_cap) return fail(c, -EIO, "adsb_process_batch: the pack step returned nonsense");
  if (nb > host_cap) {
    if ((r = ensure_pinned(c, B.h_out, (size_t)nb * sizeof(Rec), true))) return r;
    HIPCHK(c, hipMemcpyAsync(B.h_out.p, B.d_packed.p, (size_t)nb * sizeof(Rec), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  if (soft && nb > 0) {
    if ((r = ensure_pinned(c, B.h_soft_rows, (size_t)nb * sizeof(adsb_soft_fix)))) return r;
    HIPCHK(c, hipMemcpyAsync(B.h_soft_rows.p, B.d_soft_rows.p, (size_t)nb * sizeof(adsb_soft_fix), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  R->rows = (const adsb_soft_fix*)B.h_soft_rows.p;
  R->packed = (const adsb_burst*)B.h_out.p;
  R->first = h_first;
  R->kept = h_kept;
  R->nb = nb;
  int32_t nfb = 0;
  for (int32_t i = 0; i < n_items; ++i) nfb += h_kept[i] < 0 ? 1 : 0;
  R->nfb = nfb;
  if (nfb == 0) return 0;
  // The items k_batch could not finish (or was not given): each through the ordinary pass, as a blocking pass with the
  // item's plan and threshold -- enqueue / finish regrow the list capacity themselves -- and its records take the item's place.
  // The pass runs in a pipeline slot OTHER than the one adsb_last_result refers to (no slot is busy: check_batch), so the
  // previous call's records, their count and any view the caller holds into that slot's pinned buffer stay as they are; the
  // context's threshold and its list-capacity multiplier are put back afterwards (an item's density says nothing about the
  // caller's other streams).  stats.calls / stats.retries do count these passes.
  // ADSB_FLAG_FEC_SOFT_BATCH: the pass repairs as an ADSB_FLAG_FEC_SOFT context's does (soft_pass), for these passes only, and
  // the slot's rows come back with its records.
  R->fb_rows.assign((size_t)nfb, std::vector<adsb_soft_fix>());
  R->fb.assign((size_t)nfb, std::vector<adsb_burst>());
  R->fb_flags.assign((size_t)nfb, 0u);
  R->fb_of.assign((size_t)n_items, -1);
  const float thr_saved = c->thr;
  const int shift_saved = c->rec_cap_shift;
  Slot& fs = c->slot[(c->last_slot + 1) % ADSB_MAX_IN_FLIGHT];
  int32_t k = 0;
  int rc = 0;
  for (int32_t i = 0; i < n_items && rc == 0; ++i) {
    if (h_kept[i] >= 0) continue;
    Plan pl = work[(size_t)i].plan;
    pl.long_aware = long_aware;
    Summary s;
    int32_t nres = 0;
    c->thr = work[(size_t)i].thr;
    c->soft_fallback = soft;
    rc = enqueue(c, fs, pl, false);
    if (rc == 0) rc = finish(c, fs, &s, &nres);
    c->soft_fallback = false;
    if (rc == 0 && nres > 0) {
      const adsb_burst* src = (const adsb_burst*)fs.h_out.p;
      R->fb[(size_t)k].assign(src, src + nres);
      if (soft) R->fb_rows[(size_t)k].assign((const adsb_soft_fix*)fs.h_soft.p, (const adsb_soft_fix*)fs.h_soft.p + nres);
    }
    if (rc == 0) R->fb_flags[(size_t)k] = s.flags;
    R->fb_of[(size_t)i] = k++;
  }
  c->thr = thr_saved;
  c->rec_cap_shift = shift_saved;
  return rc;
}

// items[i].data: memory the device can read.  Arguments have been checked (check_batch).
int run_batch(adsb_ctx* c, int fmt, const adsb_batch_item* items, int32_t n_items, adsb_burst* out, int32_t cap,
              int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  *n_out = 0;
  item_first[0] = 0;
  if (n_fallback) *n_fallback = 0;
  if (n_items == 0) { c->batch_soft.clear(); return 0; }
  HIPCHK(c, hipSetDevice(c->device));
  int r;
  if ((r = batch_slots_ok(c, items, n_items))) return r;
  std::vector<BatchWork> work((size_t)n_items);
  for (int32_t i = 0; i < n_items; ++i) {
    work[(size_t)i].plan = plan_canonical(fmt, items[i].data, items[i].n, items[i].abs_offset, c->sps);
    work[(size_t)i].thr = items[i].threshold;
    work[(size_t)i].kind = items[i].n == 0 ? BatchWork::kEmpty : items[i].n > kBatchItemMax ? BatchWork::kHost : BatchWork::kKernel;
  }
  BatchResult R;
  if ((r = batch_core(c, fmt, work, nullptr, &R))) return r;
  if (n_fallback) *n_fallback = R.nfb;
  long long tot = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    item_first[i] = (int32_t)tot;
    tot += R.kept[i] < 0 ? (long long)R.fb[(size_t)R.fb_of[(size_t)i]].size() : (long long)(R.first[i + 1] - R.first[i]);
    if (tot >= (1ll << 31)) return fail(c, -EINVAL, "adsb_process_batch: more than 2^31 records");
  }
  item_first[n_items] = (int32_t)tot;
  *n_out = (int32_t)tot;
  if (tot > cap) return fail(c, -ENOSPC, "output array too small");
  const bool soft = (c->flags & ADSB_FLAG_FEC_SOFT_BATCH) != 0;
  if (R.nfb == 0) {
    if (tot > 0) memcpy(out, R.packed, (size_t)tot * sizeof(adsb_burst));
    if (soft) c->batch_soft.assign(R.rows, R.rows + (tot > 0 ? tot : 0));
    return 0;
  }
  if (soft) c->batch_soft.assign((size_t)tot, adsb_soft_fix{});
  for (int32_t i = 0; i < n_items; ++i) {
    const int32_t cnt = item_first[i + 1] - item_first[i];
    if (cnt == 0) continue;
    const bool fb = R.kept[i] < 0;
    const adsb_burst* src = fb ? R.fb[(size_t)R.fb_of[(size_t)i]].data() : R.packed + R.first[i];
    memcpy(out + item_first[i], src, (size_t)cnt * sizeof(adsb_burst));
    // the item's rows are spliced in with its records
    if (soft) memcpy(c->batch_soft.data() + item_first[i], fb ? R.fb_rows[(size_t)R.fb_of[(size_t)i]].data() : R.rows + R.first[i], (size_t)cnt * sizeof(adsb_soft_fix));
  }
  return 0;
}

// Host chunks into ONE device buffer, chunk i at byte offset off[i] (ascending, no overlap).  Page-locked sources are DMA'd
// where they lie; pageable ones go through the staging ring, consecutive chunks gathered into one ring chunk at their
// device spacing (by the context's copy threads, like staged_copy) and sent with one DMA -- the bytes BETWEEN two gathered
// chunks are overwritten with whatever the ring held -- (a chunk larger than a ring chunk: staged_copy, in pieces).
struct HostChunk { const void* src; size_t bytes, off; };
int upload_chunks(adsb_ctx* c, char* d, const std::vector<HostChunk>& ch) {
  constexpr size_t kRingChunk = (size_t)16 << 20;
  int rc;
  if ((rc = ensure_pool(c))) return rc;
  const hipStream_t st = c->stream;
  if ((rc = apply_ext(c, st))) return rc;
  int cur = -1;                 // ring chunk being filled, or -1
  size_t cur_lo = 0, cur_hi = 0;   // ... with the device range [cur_lo, cur_hi)
  auto flush = [&]() -> int {
    if (cur < 0) return 0;
    if (cur_hi > cur_lo) {
      HIPCHK(c, hipMemcpyAsync(d + cur_lo, c->h_ring[cur], cur_hi - cur_lo, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipEventRecord(c->ring_done[cur], st));
      c->ring_used[cur] = true;
    }
    cur = -1;
    return 0;
  };
  for (const HostChunk& h : ch) {
    const size_t bytes = h.bytes, o = h.off;
    if (bytes == 0) continue;
    if (is_pinned_host(h.src)) {
      if ((rc = flush())) return rc;
      HIPCHK(c, hipMemcpyAsync(d + o, h.src, bytes, hipMemcpyHostToDevice, st));
      continue;
    }
    if (bytes > kRingChunk) {
      if ((rc = flush())) return rc;
      if ((rc = staged_copy(c, d + o, h.src, bytes, st))) return rc;
      continue;
    }
    if (cur >= 0 && o + bytes - cur_lo > kRingChunk) { if ((rc = flush())) return rc; }
    if (cur < 0) {
      for (PinnedPtr<void>& rg : c->h_ring)
        if (!rg) HIPCHK(c, host_alloc_near(c, &rg.p, kRingChunk));
      cur = (int)(c->ring_k++ % (unsigned)adsb_ctx::kRing);
      if (c->ring_used[cur]) HIPCHK(c, hipEventSynchronize(c->ring_done[cur]));     // the chunk's previous DMA has read it
      cur_lo = o;
    }
    c->pool->copy((char*)c->h_ring[cur].p + (o - cur_lo), (const char*)h.src, bytes);     // (the context's copy threads)
    cur_hi = o + bytes;
  }
  return flush();
}

// adsb_process_batch: every item into ONE device buffer of the context (each on a 256-byte boundary).
int upload_batch(adsb_ctx* c, int fmt, const adsb_batch_item* items, int32_t n_items, std::vector<adsb_batch_item>* dev) {
  const size_t bps = (size_t)mode_bytes(fmt);
  std::vector<HostChunk> ch((size_t)n_items);
  size_t total = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    ch[(size_t)i] = HostChunk{items[i].data, (size_t)items[i].n * bps, total};
    total += ((size_t)items[i].n * bps + 255) & ~(size_t)255;
  }
  int rc;
  if ((rc = ensure(c, c->bt.d_in, total + 256))) return rc;
  char* const d = (char*)c->bt.d_in.p;
  for (int32_t i = 0; i < n_items; ++i) {
    (*dev)[(size_t)i] = items[i];
    (*dev)[(size_t)i].data = d + ch[(size_t)i].off;
  }
  return upload_chunks(c, d, ch);
}

// ---- ADSB_FLAG_STREAM_DECODE: one decoder per receiver stream, one sparse store for all of them (adsb_device.h) ---------------
FleetStore fleet_view(void* p, long long cap) {
  FleetStore v;
  v.keys = (unsigned long long*)p;
  v.ann = v.keys + cap;
  v.planes = (Plane*)(v.ann + cap);
  v.mask = (unsigned)(cap - 1);
  return v;
}
// an empty store of cap slots (a power of two), ready behind what is queued on the context's stream
// the last_seen clocks behind the planes of a flagged context's store; null without the flag
long long* fleet_seen(const adsb_ctx* c, void* p, long long cap) {
  return (c->flags & ADSB_FLAG_PLANE_AGES) ? (long long*)((char*)p + (size_t)cap * kFleetSlotBytes) : nullptr;
}
int fleet_new_store(adsb_ctx* c, DevBuf& b, long long cap) {
  const size_t bytes = (size_t)cap * (kFleetSlotBytes + ((c->flags & ADSB_FLAG_PLANE_AGES) ? sizeof(long long) : 0));
  if (hipMalloc(&b.p, bytes) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return fail(c, -ENOMEM, "stream decoders: no device memory for the store"); }
  b.cap = bytes;
  HIPCHK(c, hipMemsetAsync(b.p, 0xFF, (size_t)cap * 16, c->stream));
  HIPCHK(c, hipMemsetAsync((char*)b.p + (size_t)cap * 16, 0, (size_t)cap * sizeof(Plane), c->stream));
  return 0;
}
int fleet_take_store(adsb_ctx* c, DevBuf& fresh, long long cap) {
  FleetDec& F = c->fd;
  HIPCHK(c, F.d_store.release());
  F.d_store.p = fresh.p; F.d_store.cap = fresh.cap;
  fresh.p = nullptr; fresh.cap = 0;
  F.cap = cap;
  return 0;
}
// The live slots into a store of new_cap slots (growth, or the purge of a stream whose generations are used up): blocking.
// ADSB_FLAG_PLANE_AGES: k_ages_rehash, which moves last_seen with its slot; cutoffs ([n_streams], LLONG_MIN: keep all):
// adsb_stream_planes_expire's predicate, the dropped planes taken off the streams' books and counted in *n_removed.
int fleet_rehash(adsb_ctx* c, long long new_cap, bool renumber = false, const long long* cutoffs = nullptr, long long* n_removed = nullptr) {
  FleetDec& F = c->fd;
  const hipStream_t st = c->stream;
  const size_t ns = F.gen.size();
  int r;
  DevBuf fresh;
  if ((r = ensure(c, F.d_gen, ns * sizeof(unsigned) + sizeof(int)))) return r;
  if (cutoffs && (r = ensure(c, F.d_ages, ns * (sizeof(long long) + sizeof(FleetCount))))) return r;
  if ((r = fleet_new_store(c, fresh, new_cap))) return r;
  int* const d_err = (int*)((unsigned*)F.d_gen.p + ns);
  HIPCHK(c, hipMemcpyAsync(F.d_gen.p, F.gen.data(), ns * sizeof(unsigned), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), st));
  std::vector<FleetCount> removed;
  if (c->flags & ADSB_FLAG_PLANE_AGES) {
    FleetAges g{};
    g.from_seen = fleet_seen(c, F.d_store.p, F.cap); g.to_seen = fleet_seen(c, fresh.p, new_cap);
    if (cutoffs) {
      g.cutoffs = (const long long*)F.d_ages.p; g.removed = (FleetCount*)((long long*)F.d_ages.p + ns);
      HIPCHK(c, hipMemcpyAsync(F.d_ages.p, cutoffs, ns * sizeof(long long), hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemsetAsync(g.removed, 0, ns * sizeof(FleetCount), st));
      removed.resize(ns);
    }
    hipLaunchKernelGGL(k_ages_rehash, dim3(step_grid(F.cap, kThreads)), dim3(kThreads), 0, st, fleet_view(F.d_store.p, F.cap),
                       fleet_view(fresh.p, new_cap), (const unsigned*)F.d_gen.p, (int)ns, renumber ? 1 : 0, d_err, g);
    HIPCHK(c, hipGetLastError());
    if (cutoffs) HIPCHK(c, hipMemcpyAsync(removed.data(), g.removed, ns * sizeof(FleetCount), hipMemcpyDeviceToHost, st));
  } else {
    hipLaunchKernelGGL(k_fleet_rehash, dim3(step_grid(F.cap, kThreads)), dim3(kThreads), 0, st, fleet_view(F.d_store.p, F.cap),
                       fleet_view(fresh.p, new_cap), (const unsigned*)F.d_gen.p, (int)ns, renumber ? 1 : 0, d_err);
    HIPCHK(c, hipGetLastError());
  }
  int err = 0;
  HIPCHK(c, hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (err) return fail(c, -EIO, "stream decoders: the rehash step found the store inconsistent");
  if ((r = fleet_take_store(c, fresh, new_cap))) return r;
  long long total = 0;
  for (size_t s = 0; s < removed.size(); ++s) {
    F.slots[s] -= removed[s].slots; F.planes[s] -= removed[s].planes;
    F.live_slots -= removed[s].slots; F.live_planes -= removed[s].planes;
    total += removed[s].planes;
  }
  if (n_removed) *n_removed = total;
  F.used = F.live_slots;
  if (renumber) F.call = 1;
  return 0;
}
// a fresh decoder for stream s: its slots stay behind under the old generation until the next rehash
int fleet_reset_stream(adsb_ctx* c, size_t s) {
  FleetDec& F = c->fd;
  F.live_slots -= F.slots[s]; F.live_planes -= F.planes[s];
  F.slots[s] = F.planes[s] = 0;
  if (s == 0 && (c->flags & ADSB_FLAG_STREAM_DEDUP)) F.dd.fresh();      // (a shared decoder lives under index 0: adsb_streams_decoder_reset, adsb_reset)
  if (F.gen[s] < kFleetGenMax) { ++F.gen[s]; return 0; }
  F.gen[s] = ~0u;                               // (no key holds it: the rehash drops every slot of the stream)
  HIPCHK(c, hipSetDevice(c->device));
  const int r = fleet_rehash(c, F.cap);
  F.gen[s] = 0;
  return r;
}
int fleet_open(adsb_ctx* c, size_t n) {
  FleetDec& F = c->fd;
  DevBuf fresh;
  int r;
  if ((r = fleet_new_store(c, fresh, kFleetDefaultCap)) || (r = fleet_take_store(c, fresh, kFleetDefaultCap))) return r;
  F.start.assign(n, 0.0); F.gen.assign(n, 0u); F.slots.assign(n, 0); F.planes.assign(n, 0);
  F.used = F.live_slots = F.live_planes = F.grows = 0;
  F.call = 0; F.n_rows = 0; F.all = 1;
  F.dd.fresh(); F.dd.window = 0.002; F.dd.horizon = 1.0; F.dd.cur = 0;
  F.rx.assign(3 * n, std::numeric_limits<double>::quiet_NaN());
  F.open = true;
  return 0;
}
int fleet_close(adsb_ctx* c) {
  FleetDec& F = c->fd;
  F.open = false; F.cap = 0; F.n_rows = 0;
  F.start.clear(); F.gen.clear(); F.slots.clear(); F.planes.clear(); F.rx.clear();
  F.trk.cur = F.trk.n = 0;
  for (DevBuf* b : {&F.d_store, &F.d_recs, &F.d_items, &F.d_cnt, &F.d_keys, &F.d_sorted, &F.d_tmp, &F.d_ts, &F.d_rows, &F.d_gen, &F.d_snap, &F.d_ages, &F.d_merged, &F.d_shared, &F.dd.d_carry[0], &F.dd.d_carry[1], &F.dd.d_call, &F.d_mlat, &F.trk.d_rows[0], &F.trk.d_rows[1], &F.trk.d_work}) HIPCHK(c, b->release());
  for (PinnedBuf* b : {&F.h_recs, &F.h_rows, &F.h_items, &F.h_cnt, &F.h_shared, &F.h_order, &F.h_order_next, &F.dd.h_dup, &F.dd.h_dup_next, &F.h_mlat, &F.trk.h_cnt}) HIPCHK(c, b->release());
  return 0;
}

// The decode step of one delivered call: recs[0 .. n) is its final list (item i: [item_first[i], item_first[i + 1])).  The
// records come back in F.h_recs with their verdict flags, the rows in F.h_rows.  Everything that can fail for want of
// memory happens before the first kernel that touches the store.
// ADSB_FLAG_STREAM_DECODE_SHARED: one decoder for all streams.  The list is put into the order ascending (timestamp, list
// position) first (adsb_shared.hip), the same kernels run on that list as ONE item of stream 0, and the verdict flags and
// rows go back to list positions; F.h_order holds the order of the last call that was delivered (a call that fails here leaves it).
// ADSB_FLAG_STREAM_DEDUP (include/adsb_hip.h: DE-DUPLICATION): between the gather and k_fleet_announce the duplicates lose
// ADSB_BURST_DEMOD in the time-ordered copy, and the call's entries are merged with the carry into the carry's other buffer;
// behind the scatter the duplicates' delivered records and rows are marked.  The cut's {offset, count, hi} comes down behind
// the counts in h_cnt; the host takes it, and the other buffer, only when the call is delivered.
int fleet_step(adsb_ctx* c, const adsb_stream_item* items, int32_t n_items, const int32_t* item_first, const adsb_burst* recs, int32_t n) {
  FleetDec& F = c->fd;
  const hipStream_t st = c->stream;
  if (n == 0) { F.n_rows = 0; return 0; }
  int r;
  const bool shared = (c->flags & ADSB_FLAG_STREAM_DECODE_SHARED) != 0;
  const size_t nn = (size_t)n, ni = shared ? 1 : (size_t)n_items;      // ni: the items of the decode step's own table
  const int nblk = (int)((nn + kSortTile - 1) / kSortTile);
  const bool dedup = shared && (c->flags & ADSB_FLAG_STREAM_DEDUP) != 0;
  FleetDec::Dedup& D = F.dd;
  // first[n_items + 1] | start[n_items] (| the items' streams[n_items])
  const size_t shared_tab = ((size_t)n_items + 1) * sizeof(int) + (size_t)n_items * sizeof(double) + (dedup ? (size_t)n_items * sizeof(int) : 0);
  const size_t dd_dup = nn * adsb_dedup_host::kEntBytes, dd_streams = dd_dup + ((nn * sizeof(int) + 255) & ~(size_t)255);
  if (dedup && ((r = ensure(c, D.d_call, dd_streams + (size_t)n_items * sizeof(int))) ||
                (r = ensure(c, D.d_carry[D.cur ^ 1], ((size_t)D.cnt + nn) * adsb_dedup_host::kEntBytes)) ||
                (r = ensure_pinned(c, D.h_dup_next, nn * sizeof(int)))))
    return r;
  if (dedup && (long long)D.cnt + n >= (1ll << 31)) return fail(c, -ENOMEM, "shared decoder: the de-duplication carry would exceed 2^31 entries");
  if (shared && ((r = ensure(c, F.d_shared, SharedBufs::bytes(nn, (size_t)n_items))) || (r = ensure_pinned(c, F.h_shared, shared_tab)) ||
                 (r = ensure_pinned(c, F.h_order_next, nn * sizeof(int)))))
    return r;
  const size_t cnt_head = ni * sizeof(FleetCount) + (ni + 2) * sizeof(int), dd_state = (cnt_head + 7) & ~(size_t)7;
  const size_t cnt_bytes = dedup ? dd_state + sizeof(adsb_dedup_host::State) : cnt_head;
  if ((r = ensure(c, F.d_recs, nn * sizeof(Rec))) || (r = ensure(c, F.d_items, (ni + 1) * sizeof(FleetItem))) ||
      (r = ensure(c, F.d_cnt, cnt_bytes)) || (r = ensure(c, F.d_keys, nn * 8)) || (r = ensure(c, F.d_sorted, nn * 8)) ||
      (r = ensure(c, F.d_tmp, (size_t)nblk * 16 * sizeof(unsigned))) || (r = ensure(c, F.d_ts, nn * 8)) || (r = ensure(c, F.d_rows, nn * sizeof(DecRow))) ||
      (r = ensure_pinned(c, F.h_recs, nn * sizeof(Rec))) || (r = ensure_pinned(c, F.h_rows, nn * sizeof(DecRow))) ||
      (r = ensure_pinned(c, F.h_items, (ni + 1) * sizeof(FleetItem))) || (r = ensure_pinned(c, F.h_cnt, cnt_bytes)))
    return r;
  // Room for one slot per record with at most half the store taken, or a rehash first: it drops the slots reset streams left
  // behind, into a store that is larger only if the LIVE slots need it (a growth).  The call numbers of the ordering keys
  // start over at such a rehash before they run out.
  const bool renumber = F.call >= 0xFFFFFFFEull;
  if ((F.used + n) * 2 > F.cap || renumber) {
    const long long old_cap = F.cap;
    long long cap = old_cap;
    while ((F.live_slots + n) * 2 > cap) cap *= 2;
    if (cap > kFleetMaxCap) return fail(c, -ENOMEM, "stream decoders: the store would exceed 2^27 slots");
    if ((r = fleet_rehash(c, cap, renumber))) return r;
    if (cap > old_cap) F.grows++;
  }
  FleetItem* const hi = (FleetItem*)F.h_items.p;
  SharedBufs sh;
  if (shared) {                                  // the whole list is one item of stream 0 (its start is not used: see d_ts below)
    sh = SharedBufs(F.d_shared.p, nn, (size_t)n_items);
    hi[0].first = 0; hi[0].stream = 0; hi[0].base = (unsigned long long)F.gen[0] << (kFleetAddrBits + kFleetStreamBits); hi[0].start = 0;
    int* const hf = (int*)F.h_shared.p;
    double* const hs = (double*)(hf + n_items + 1);
    for (int32_t i = 0; i < n_items; ++i) {
      hf[i] = item_first[i];
      const double start = F.start[(size_t)items[i].stream];
      memcpy(&hs[i], &start, sizeof(double));    // (behind an odd number of ints: not aligned)
    }
    hf[n_items] = n;
  } else
    for (int32_t i = 0; i < n_items; ++i) {
      const size_t s = (size_t)items[i].stream;
      hi[i].first = item_first[i];
      hi[i].stream = items[i].stream;
      hi[i].base = ((unsigned long long)F.gen[s] << (kFleetAddrBits + kFleetStreamBits)) | ((unsigned long long)s << kFleetAddrBits);
      hi[i].start = F.start[s];
    }
  hi[ni].first = n; hi[ni].stream = -1; hi[ni].base = 0; hi[ni].start = 0;
  memcpy(F.h_recs.p, recs, nn * sizeof(Rec));
  HIPCHK(c, hipMemcpyAsync(F.d_recs.p, F.h_recs.p, nn * sizeof(Rec), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(F.d_items.p, hi, (ni + 1) * sizeof(FleetItem), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(F.d_cnt.p, 0, cnt_bytes, st));
  if (shared) {
    HIPCHK(c, hipMemcpyAsync(sh.first, F.h_shared.p, ((size_t)n_items + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(sh.start, (const char*)F.h_shared.p + ((size_t)n_items + 1) * sizeof(int), (size_t)n_items * sizeof(double),
                             hipMemcpyHostToDevice, st));
    hipError_t e;
    if ((e = (hipError_t)adsb_shared_host::launch_keys(st, F.d_recs.p, n, sh.first, sh.start, n_items, c->fs, sh.keys, sh.vals, sh.ts)) ||
        (e = (hipError_t)adsb_shared_host::launch_sort(st, sh.keys, sh.vals, sh.keys_tmp, sh.vals_tmp, n, sh.hist)) ||
        (e = (hipError_t)adsb_shared_host::launch_gather(st, F.d_recs.p, sh.ts, sh.vals, n, sh.recs, sh.ts_sorted, sh.order)))
      return fail(c, -EIO, "shared decoder: the time order's kernels", e);
    if (dedup) {
      char* const call = (char*)D.d_call.p;
      int* const hstreams = (int*)((char*)F.h_shared.p + ((size_t)n_items + 1) * sizeof(int) + (size_t)n_items * sizeof(double));
      for (int32_t i = 0; i < n_items; ++i) hstreams[i] = items[i].stream;
      HIPCHK(c, hipMemcpyAsync(call + dd_streams, hstreams, (size_t)n_items * sizeof(int), hipMemcpyHostToDevice, st));
      const char* const carry = (const char*)D.d_carry[D.cur].p + (size_t)D.off * adsb_dedup_host::kEntBytes;     // (null while cnt == 0: never read)
      if ((e = (hipError_t)adsb_dedup_host::launch_entries(st, sh.recs, sh.ts_sorted, sh.order, n, sh.first, (const int*)(call + dd_streams),
                                                           n_items, call)) ||
          (e = (hipError_t)adsb_dedup_host::launch_find(st, call, n, carry, D.cnt, D.window, sh.order, sh.recs, (int*)(call + dd_dup))) ||
          (e = (hipError_t)adsb_dedup_host::launch_merge(st, carry, D.cnt, call, n, D.horizon, D.d_carry[D.cur ^ 1].p,
                                                         (char*)F.d_cnt.p + dd_state)))
        return fail(c, -EIO, "shared decoder: the de-duplication kernels", e);
    }
  }
  FleetArgs a{};
  a.recs = shared ? sh.recs : (Rec*)F.d_recs.p; a.n = n; a.n_items = (int)ni; a.items = (const FleetItem*)F.d_items.p;
  a.count = (FleetCount*)F.d_cnt.p; a.ncond = (int*)(a.count + ni); a.error = a.ncond + ni + 1;
  a.s = fleet_view(F.d_store.p, F.cap);
  a.call = F.call << 32;
  a.fec = (c->flags & ADSB_FLAG_FEC_CONSERVATIVE) ? 1 : 0; a.all = F.all; a.fs = c->fs;
  a.keys = (unsigned long long*)F.d_keys.p; a.sorted = (const unsigned long long*)F.d_sorted.p;
  a.rows = shared ? sh.rows : (DecRow*)F.d_rows.p;
  a.ts = (double*)F.d_ts.p; a.seen = fleet_seen(c, F.d_store.p, F.cap);
  const unsigned g = step_grid(n, kThreads);
  hipLaunchKernelGGL(k_fleet_announce, dim3(g), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(k_fleet_verdict, dim3(g), dim3(kThreads), 0, st, a, 0);
  hipLaunchKernelGGL(k_fleet_cond, dim3((unsigned)ni), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_fleet_verdict, dim3(g), dim3(kThreads), 0, st, a, 1);
  hipLaunchKernelGGL(k_fleet_classify, dim3(g), dim3(kThreads), 0, st, a);
  // k_fleet_classify's timestamps are start + offset / fs with the ONE item's start: the true ones, in time order, over them
  if (shared) HIPCHK(c, hipMemcpyAsync(F.d_ts.p, sh.ts_sorted, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
  launch_key_sort(st, (unsigned long long*)F.d_keys.p, (unsigned long long*)F.d_sorted.p, (int)n, 32, 60, (unsigned*)F.d_tmp.p);      // as launch_dec
  hipLaunchKernelGGL(k_fleet_fold, dim3((unsigned)((nn + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);     // one thread per key
  HIPCHK(c, hipGetLastError());
  if (shared) {
    hipError_t e2;
    const hipError_t e = (hipError_t)adsb_shared_host::launch_scatter(st, sh.recs, sh.rows, sh.order, n, F.d_recs.p, F.d_rows.p);
    if (e) return fail(c, -EIO, "shared decoder: k_shared_scatter", e);
    HIPCHK(c, hipMemcpyAsync(F.h_order_next.p, sh.order, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    if (dedup) {
      const int* const dup = (const int*)((const char*)D.d_call.p + dd_dup);
      if ((e2 = (hipError_t)adsb_dedup_host::launch_mark(st, dup, n, F.d_recs.p, F.d_rows.p))) return fail(c, -EIO, "shared decoder: k_dedup_mark", e2);
      HIPCHK(c, hipMemcpyAsync(D.h_dup_next.p, dup, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(c, hipMemcpyAsync(F.h_recs.p, F.d_recs.p, nn * sizeof(Rec), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(F.h_rows.p, F.d_rows.p, nn * sizeof(DecRow), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(F.h_cnt.p, F.d_cnt.p, cnt_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const FleetCount* const hc = (const FleetCount*)F.h_cnt.p;
  if (((const int*)(hc + ni))[ni + 1] != 0) return fail(c, -EIO, "stream decoders: the decode step found the store inconsistent");
  adsb_dedup_host::State ds{};
  if (dedup) {                                   // before anything is committed: a call that fails leaves order[], dup[] and the carry alone
    memcpy(&ds, (const char*)F.h_cnt.p + dd_state, sizeof ds);
    if (ds.off < 0 || ds.cnt < 1 || (long long)ds.off + ds.cnt != (long long)D.cnt + n) return fail(c, -EIO, "shared decoder: the de-duplication carry's cut is inconsistent");
  }
  for (size_t i = 0; i < ni; ++i) {
    const size_t s = shared ? 0 : (size_t)items[i].stream;
    F.slots[s] += hc[i].slots; F.planes[s] += hc[i].planes;
    F.live_slots += hc[i].slots; F.live_planes += hc[i].planes; F.used += hc[i].slots;
  }
  F.call++;
  F.n_rows = n;
  if (shared) { std::swap(F.h_order.p, F.h_order_next.p); std::swap(F.h_order.cap, F.h_order_next.cap); }      // delivered
  if (dedup) {
    std::swap(D.h_dup.p, D.h_dup_next.p); std::swap(D.h_dup.cap, D.h_dup_next.cap);
    const int* const dup = (const int*)D.h_dup.p;
    for (size_t t = 0; t < nn; ++t) D.duplicates += dup[t] != -1;
    D.cur ^= 1; D.off = ds.off; D.cnt = ds.cnt; D.hi = ds.hi; D.delivered = true;
  }
  return 0;
}

// ---- adsb_process_stream_batch*: receiver streams carried across batch calls -------------------------------------------------
// One call pushes the next chunk of any subset of the context's streams through ONE k_batch launch: item i is one overlapped
// time shard of its stream (adsb_plan.h: plan_stream_item) whose gate starts from the stream's carried end-of-burst offset.
// Around the launch, k_stream_stage assembles each item's buffer [stream carry | new chunk] in d_stage and k_stream_save keeps
// the buffer's last samples for the next call.  A stream's carry has two slots: the save step writes the one the stage step
// did not read, and the host flips them when the call's records are delivered -- so a call that fails (-ENOSPC) has moved
// nothing and can be repeated.
int check_stream_batch(adsb_ctx* c, int fmt, const adsb_stream_item* items, int32_t n_items, bool device, adsb_burst* out,
                       int32_t cap, int32_t* item_first, int32_t* n_out) {
  if (!c) return -EINVAL;
  if (fmt < 0 || fmt >= ADSB_FMT_COUNT) return fail(c, -EINVAL, "adsb_process_stream_batch: bad format");
  if (n_items < 0 || (n_items > 0 && !items) || cap < 0 || (cap > 0 && !out) || !item_first || !n_out)
    return fail(c, -EINVAL, "adsb_process_stream_batch: bad argument");
  if (c->flags & (ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE | ADSB_FLAG_CONFIDENCE))
    return fail(c, -EINVAL, "adsb_process_stream_batch: not for ADSB_FLAG_AIRCRAFT_TABLE / _DECODE / _CONFIDENCE contexts (one receiver each)");
  if (c->flags & ADSB_FLAG_FEC_SOFT) return fail(c, -EINVAL, "adsb_process_stream_batch: not for ADSB_FLAG_FEC_SOFT contexts");
  StreamBufs& S = c->sb;
  if (S.st.empty()) return fail(c, -EINVAL, "adsb_process_stream_batch: no streams (adsb_streams_open first)");
  const uintptr_t unit = (uintptr_t)mode_bytes(fmt);
  std::vector<char> seen(S.st.size(), 0);
  for (int32_t i = 0; i < n_items; ++i) {
    const adsb_stream_item& it = items[i];
    if (it.reserved != 0u || (it.flags & ~ADSB_STREAM_END)) return fail(c, -EINVAL, "adsb_process_stream_batch: item.reserved / unknown item.flags must be 0");
    if (it.n < 0) return fail(c, -EINVAL, "adsb_process_stream_batch: item.n < 0");
    if (it.n > 0 && !it.data) return fail(c, -EINVAL, "adsb_process_stream_batch: item.data is NULL");
    if (device && it.n > 0 && ((uintptr_t)it.data % unit) != 0) return fail(c, -EINVAL, "adsb_process_stream_batch: item.data must be aligned to a sample");
    if (it.stream < 0 || (size_t)it.stream >= S.st.size()) return fail(c, -EINVAL, "adsb_process_stream_batch: no such stream");
    if (seen[(size_t)it.stream]) return fail(c, -EINVAL, "adsb_process_stream_batch: a stream appears twice in one call");
    seen[(size_t)it.stream] = 1;
    const StreamState& s = S.st[(size_t)it.stream];
    if (s.pos > 0 && s.fmt != fmt) return fail(c, -EINVAL, "adsb_process_stream_batch: the stream started with another format");
  }
  return require_idle(c, kCallPending);
}

int run_stream_batch(adsb_ctx* c, int fmt, const adsb_stream_item* items, int32_t n_items, bool device, adsb_burst* out, int32_t cap,
                     int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  *n_out = 0;
  item_first[0] = 0;
  if (n_fallback) *n_fallback = 0;
  if (n_items == 0) { c->fd.n_rows = 0; c->batch_soft.clear(); return 0; }
  HIPCHK(c, hipSetDevice(c->device));
  StreamBufs& S = c->sb;
  const hipStream_t st = c->stream;
  const int sps = c->sps, bps = mode_bytes(fmt);
  int r;
  // every item's buffer on a 256-byte boundary of the staging buffer
  std::vector<StreamItem> plan((size_t)n_items);
  std::vector<size_t> off((size_t)n_items);
  size_t total = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    const StreamState& s = S.st[(size_t)items[i].stream];
    plan[(size_t)i] = plan_stream_item(fmt, s.pos, items[i].n, (items[i].flags & ADSB_STREAM_END) != 0, s.base, s.eob, sps);
    off[(size_t)i] = total;
    total += ((size_t)plan[(size_t)i].n_buf * (size_t)bps + 255) & ~(size_t)255;
  }
  const size_t tab_bytes = (size_t)n_items * (sizeof(StreamStage) + sizeof(StreamSave));
  if ((r = ensure(c, S.d_stage, total + 256))) return r;
  if ((r = ensure(c, S.d_tab, tab_bytes))) return r;
  if ((r = ensure_pinned(c, S.h_tab, tab_bytes))) return r;
  if ((r = ensure_pinned(c, S.h_status, (size_t)n_items * sizeof(StreamStatus), true))) return r;
  char* const d = (char*)S.d_stage.p;
  StreamStage* const hsg = (StreamStage*)S.h_tab.p;
  StreamSave* const hsv = (StreamSave*)(hsg + n_items);
  std::vector<BatchWork> work((size_t)n_items);
  std::vector<HostChunk> ch;
  for (int32_t i = 0; i < n_items; ++i) {
    const StreamState& s = S.st[(size_t)items[i].stream];
    StreamItem& it = plan[(size_t)i];
    char* const slot = (char*)S.d_carry.p + (size_t)items[i].stream * 2 * S.slot_bytes;
    fill_stream_copies(hsg[i], hsv[i], it, s.pos, items[i].n, sps, bps, d + off[(size_t)i], slot + (size_t)s.cur * S.slot_bytes,
                       slot + (size_t)(s.cur ^ 1) * S.slot_bytes, device && items[i].n > 0 ? items[i].data : nullptr);
    if (!device) ch.push_back(HostChunk{items[i].data, (size_t)items[i].n * (size_t)bps, (size_t)((char*)hsg[i].chunk.dst - d)});
    it.plan.d_data = d + off[(size_t)i];
    work[(size_t)i].plan = it.plan;
    work[(size_t)i].thr = items[i].threshold;
    work[(size_t)i].kind = !it.run ? BatchWork::kEmpty : it.n_buf > kBatchItemMax ? BatchWork::kHost : BatchWork::kKernel;
  }
  // the host entry point's chunks go straight into place: only the carries are copied on the device
  if (!device && (r = upload_chunks(c, d, ch))) return r;
  if ((r = apply_ext(c, st))) return r;
  HIPCHK(c, hipMemcpyAsync(S.d_tab.p, S.h_tab.p, tab_bytes, hipMemcpyHostToDevice, st));
  StreamStatus* const status = (StreamStatus*)S.h_status.p;
  const StreamHooks hooks{(const StreamStage*)S.d_tab.p, (const StreamSave*)((const StreamStage*)S.d_tab.p + n_items), status};
  BatchResult R;
  if ((r = batch_core(c, fmt, work, &hooks, &R))) return r;
  if (n_fallback) *n_fallback = R.nfb;
  // what each item delivers and where its stream stands afterwards (adsb_plan.h: stream_deliver) -- nothing is committed yet
  size_t room = (size_t)R.nb + 1;
  for (const std::vector<adsb_burst>& f : R.fb) room += f.size();
  std::vector<adsb_burst> keep(room);
  const bool soft = (c->flags & ADSB_FLAG_FEC_SOFT_BATCH) != 0;
  std::vector<adsb_soft_fix> keep_rows(soft ? room : 0);
  std::vector<StreamState> next((size_t)n_items);
  long long tot = 0;
  for (int32_t i = 0; i < n_items; ++i) {
    const bool fb = R.kept[i] < 0;
    const std::vector<adsb_burst>* f = fb ? &R.fb[(size_t)R.fb_of[(size_t)i]] : nullptr;
    const adsb_burst* src = fb ? f->data() : R.packed + R.first[i];
    const int cnt = fb ? (int)f->size() : R.first[i + 1] - R.first[i];
    const unsigned sum_flags = fb ? R.fb_flags[(size_t)R.fb_of[(size_t)i]] : status[i].flags;
    if (!fb && status[i].kept != R.kept[i]) return fail(c, -EIO, "adsb_process_stream_batch: the save step returned nonsense");
    StreamState n = S.st[(size_t)items[i].stream];
    const int w = stream_deliver(src, cnt, keep.data() + tot, plan[(size_t)i].plan, sum_flags, sps,
                                 [](const adsb_burst& b) { return (long long)b.offset; },
                                 [](const adsb_burst& b) { return (unsigned)b.flags; }, &n.eob, &n.overlong);
    if (soft) {
      // Rows are dropped with their records, so row t stays with delivered record t: what stream_deliver kept is a subsequence
      // of src in order, found again by comparing whole records.  A repair changes neither offset, DF nor length (bits 0-4 are
      // never candidates), so the drops, the carried gate state (eob) and ADSB_BURST_LONG_HINT are what they are without the flag.
      const adsb_soft_fix* rows = fb ? R.fb_rows[(size_t)R.fb_of[(size_t)i]].data() : R.rows + R.first[i];
      int t = 0;
      for (int j = 0; j < cnt && t < w; ++j)
        if (memcmp(&src[j], &keep[(size_t)(tot + t)], sizeof(adsb_burst)) == 0) keep_rows[(size_t)(tot + t++)] = rows[j];
      if (t != w) return fail(c, -EIO, "adsb_process_stream_batch: the delivered records are not a subsequence of the pass's");
    }
    item_first[i] = (int32_t)tot;
    tot += w;
    if (tot >= (1ll << 31)) return fail(c, -EINVAL, "adsb_process_stream_batch: more than 2^31 records");
    n.cur ^= 1;
    n.fmt = fmt;
    if (items[i].flags & ADSB_STREAM_END) { n.pos = 0; n.eob = kStreamFreshEob; n.fmt = -1; }
    else n.pos += items[i].n;
    next[(size_t)i] = n;
  }
  item_first[n_items] = (int32_t)tot;
  *n_out = (int32_t)tot;
  if (tot > cap) return fail(c, -ENOSPC, "output array too small");
  const adsb_burst* fin = keep.data();
  if (c->flags & ADSB_FLAG_STREAM_DECODE) {      // the call is delivered: every stream's decoder takes its records
    if ((r = fleet_step(c, items, n_items, item_first, keep.data(), (int32_t)tot))) return r;
    fin = (const adsb_burst*)c->fd.h_recs.p;
  }
  if (tot > 0) memcpy(out, fin, (size_t)tot * sizeof(adsb_burst));
  if (soft) c->batch_soft.assign(keep_rows.begin(), keep_rows.begin() + tot);
  for (int32_t i = 0; i < n_items; ++i) S.st[(size_t)items[i].stream] = next[(size_t)i];
  return 0;
}

}  // namespace

extern "C" {

int adsb_abi_version(void) { return ADSB_ABI_VERSION; }

int32_t adsb_plan_chunks(int64_t n_samples, int64_t resident_wavefronts, int64_t* units, int64_t* samples_per_chunk) {
  if (n_samples < 0 || resident_wavefronts < 1 || !units || !samples_per_chunk) return -EINVAL;
  long long u = 0, t = 0;
  plan_chunks((n_samples + kWTile - 1) / kWTile, resident_wavefronts, &u, &t);
  *units = u; *samples_per_chunk = t * kWTile;
  return 0;
}

uint32_t adsb_mode_s_syndrome(const uint8_t bits[14], int32_t* df_out, int32_t* nbits_out) {
  // decoder.py:551 (DF), :565,604,636,669 (format sets), :693-714 (compute_crc); same table as the device
  static constexpr CrcTab tab = make_crc_tab();
  const unsigned df = bits[0] >> 3, dfb = 1u << df;
  const bool lng = (dfb & kDfLongSet) != 0, known = lng || (dfb & kDfShortSet) != 0;
  const int L = lng ? 112 : 56;
  uint32_t syn = 0;
  for (int i = 0; i < L; ++i)
    if ((bits[i >> 3] >> (7 - (i & 7))) & 1) syn ^= tab.r[L - 1 - i];
  if (df_out) *df_out = (int32_t)df;
  if (nbits_out) *nbits_out = known ? L : 0;
  return syn;
}

// pre-filter flags of one payload (the device's parity_flags_of, from adsb_mode_s_syndrome)
static uint32_t host_parity_flags(const uint8_t b[14]) {
  int32_t df = 0, nbits = 0;
  const uint32_t syn = adsb_mode_s_syndrome(b, &df, &nbits);
  uint32_t f = (uint32_t)df << ADSB_BURST_DF_SHIFT;
  if (nbits == 112) f |= ADSB_BURST_LONG;
  if (nbits) f |= ADSB_BURST_KNOWN_DF;
  if (((1u << df) & kDfPiSet) && syn == 0) f |= ADSB_BURST_PARITY_OK;
  return f;
}

// decoder.py:304-323: for burst lengths 1, 2 and every position, key = compute_crc_2 of the pattern; :738-763: the payload's
// key looked up.  compute_crc_2(bits[0:L]) (:716-736) is the L-bit message mod x*G(x) -- 25 bits.  Returns whether a pattern
// matches; *first / *len = the pattern, e = the payload with it applied.
static bool host_fec_find(const uint8_t b[14], int L, int32_t* first, int32_t* len, uint8_t e[14]) {
  static constexpr CrcTab tab = make_crc_tab();
  auto key = [](const uint8_t* v, int n) {        // sum over set bits i of x^(n-1-i) mod x*G = x * (x^(n-2-i) mod G), or 1
    uint32_t k = 0;
    for (int i = 0; i < n; ++i)
      if ((v[i >> 3] >> (7 - (i & 7))) & 1) k ^= (i == n - 1) ? 1u : (tab.r[n - 2 - i] << 1);
    return k;
  };
  const uint32_t k = key(b, L);
  for (int w = 1; w <= 2; ++w)
    for (int i = 0; i + w <= L; ++i) {
      uint8_t p[14] = {0};
      for (int q = i; q < i + w; ++q) p[q >> 3] |= (uint8_t)(0x80u >> (q & 7));
      if (key(p, L) != k) continue;
      *first = i;
      *len = w;
      for (int q = 0; q < 14; ++q) e[q] = (uint8_t)(p[q] ^ b[q]);
      return true;
    }
  return false;
}

uint32_t adsb_mode_s_fec(const uint8_t in[14], uint8_t out[14], int32_t* first_bit, int32_t* nflip) {
  uint8_t b[14];
  memcpy(b, in, 14);
  if (first_bit) *first_bit = -1;
  if (nflip) *nflip = 0;
  const uint32_t flags = host_parity_flags(b);
  const unsigned df = b[0] >> 3;
  if (out) memcpy(out, b, 14);
  if (!((1u << df) & kDfPiSet) || (flags & ADSB_BURST_PARITY_OK)) return flags;
  const int L = (flags & ADSB_BURST_LONG) ? 112 : 56;
  int32_t i = 0, len = 0;
  uint8_t e[14];
  if (!host_fec_find(b, L, &i, &len, e)) return flags;
  if (first_bit) *first_bit = i;
  if (nflip) *nflip = len;
  const uint32_t f2 = host_parity_flags(e);
  const unsigned df2 = e[0] >> 3;
  if (((1u << df2) & kDfPiSet) && ((f2 & ADSB_BURST_LONG) == (flags & ADSB_BURST_LONG))) {
    if (out) memcpy(out, e, 14);
    return f2 | ADSB_BURST_FEC_FIXED;
  }
  return flags | ADSB_BURST_FEC_DF;
}

// decode_message / decode_me (decoder.py:883-947,1065-1232) as far as they reach update_plane for a reply that passed:
// the address it announces, or -1
static int32_t host_announce(const uint8_t b[14]) {
  auto field = [&](int lo, int n) {
    uint32_t v = 0;
    for (int i = lo; i < lo + n; ++i) v = (v << 1) | ((b[i >> 3] >> (7 - (i & 7))) & 1u);
    return v;
  };
  const uint32_t df = field(0, 5), sub = field(5, 3), tc = field(32, 5), st = field(37, 3);
  const int32_t aa = (int32_t)field(8, 24);
  if (df == 11) return aa;                                                     // :883-893
  if (df == 17 || (df == 18 && (sub == 0 || sub == 1 || sub == 6)) || (df == 19 && sub == 0)) {   // :896-947 -> decode_me
    if ((tc >= 1 && tc <= 4) || (tc >= 9 && tc <= 18)) return aa;            // :1075-1088, :1100-1112
    if (tc == 19 && (st == 1 || st == 2)) return aa;                           // :1141-1232
  }
  return -1;
}

uint32_t adsb_mode_s_aircraft(const uint8_t bits[14], int32_t fec, int32_t* aa_out, int32_t* announce, int32_t* fec_announce) {
  int32_t aa = -1, ann = -1, fann = -1;
  uint32_t ret = 0;
  int32_t df = 0, nbits = 0;
  const uint32_t syn = adsb_mode_s_syndrome(bits, &df, &nbits);
  const uint32_t ap_set = (1u << 0) | (1u << 4) | (1u << 5) | (1u << 16) | (1u << 20) | (1u << 21) | (1u << 24);
  int32_t i = 0, len = 0;
  uint8_t e[14];
  if ((1u << df) & ap_set) {
    // check_parity (:576-601, :636-665): AA = crc ^ AP = the syndrome; unknown: correct_burst_errors on the raw reply,
    // keyed by (AA, last bit); decode_message then runs on the repaired bits with self.aa_str of check_parity
    aa = (int32_t)syn;
    if (fec && host_fec_find(bits, nbits, &i, &len, e)) {
      ret = ADSB_BURST_AP_FEC;
      const uint32_t df2 = e[0] >> 3;
      fann = (((1u << df2) & ap_set) && df2 != 24) ? aa : host_announce(e);
    }
  } else if ((1u << df) & kDfPiSet) {
    if (syn == 0) ann = host_announce(bits);
    else if (fec && host_fec_find(bits, nbits, &i, &len, e)) ann = host_announce(e);   // the decoder's own repair
  }
  if (aa_out) *aa_out = aa;
  if (announce) *announce = ann;
  if (fec_announce) *fec_announce = fann;
  return ret;
}

// WGS-84
static constexpr double kWgsA = 6378137.0, kWgsF = 1.0 / 298.257223563, kWgsE2 = kWgsF * (2.0 - kWgsF), kWgsB = kWgsA * (1.0 - kWgsF);
static constexpr double kRadPerDeg = 3.14159265358979323846 / 180.0;

void adsb_geodetic_to_ecef(double lat_deg, double lon_deg, double alt_m, double* x, double* y, double* z) {
  const double lat = lat_deg * kRadPerDeg, lon = lon_deg * kRadPerDeg;
  const double sl = std::sin(lat), cl = std::cos(lat);
  const double n = kWgsA / std::sqrt(1.0 - kWgsE2 * sl * sl);
  if (x) *x = (n + alt_m) * cl * std::cos(lon);
  if (y) *y = (n + alt_m) * cl * std::sin(lon);
  if (z) *z = (n * (1.0 - kWgsE2) + alt_m) * sl;
}

void adsb_ecef_to_geodetic(double x, double y, double z, double* lat_deg, double* lon_deg, double* alt_m) {
  const double p = std::sqrt(x * x + y * y);
  const double ep2 = kWgsE2 / (1.0 - kWgsE2);
  const double th = std::atan2(z * kWgsA, p * kWgsB);                 // Bowring's start
  double st = std::sin(th), ct = std::cos(th);
  double lat = std::atan2(z + ep2 * kWgsB * st * st * st, p - kWgsE2 * kWgsA * ct * ct * ct);
  for (int k = 0; k < 3; ++k) {                                       // lat = atan2(z + e^2 N sin lat, p)
    const double sl = std::sin(lat);
    const double n = kWgsA / std::sqrt(1.0 - kWgsE2 * sl * sl);
    lat = std::atan2(z + kWgsE2 * n * sl, p);
  }
  const double sl = std::sin(lat), cl = std::cos(lat);
  const double n = kWgsA / std::sqrt(1.0 - kWgsE2 * sl * sl);
  // the height along the normal, by whichever of the two projections is the better conditioned
  const double alt = std::fabs(cl) > 0.5 ? p / cl - n : z / sl - n * (1.0 - kWgsE2);
  if (lat_deg) *lat_deg = lat / kRadPerDeg;
  if (lon_deg) *lon_deg = p > 0.0 ? std::atan2(y, x) / kRadPerDeg : 0.0;
  if (alt_m) *alt_m = alt;
}

float adsb_snr_db(float peak, float median) {
  // framer.py:157 under NumPy-2 promotion: every operation in float32
  volatile float q = peak / median;
  volatile float l = log10f(q);
  volatile float m = 10.0f * l;
  volatile float r = m + 1.6f;
  return r;
}

int adsb_create(double fs, float threshold, int device, uint32_t flags, adsb_ctx** out) {
  if ((flags & ADSB_FLAG_DECODE) && !(flags & ADSB_FLAG_AIRCRAFT_TABLE)) return -EINVAL;   // the decode step follows the table's
  if ((flags & ADSB_FLAG_STREAM_DECODE) && (flags & (ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE | ADSB_FLAG_CONFIDENCE))) return -EINVAL;
  if ((flags & ADSB_FLAG_PLANE_AGES) && !(flags & (ADSB_FLAG_DECODE | ADSB_FLAG_STREAM_DECODE))) return -EINVAL;   // no planes to age
  if ((flags & ADSB_FLAG_FEC_SOFT) && (flags & (ADSB_FLAG_STREAM_DECODE | ADSB_FLAG_FRAMER_SLICES))) return -EINVAL;   // one receiver's records; no pairing
  // the batch form: one meaning of "soft" per context, and none of the contexts the batch entry points refuse anyway
  if ((flags & ADSB_FLAG_FEC_SOFT_BATCH) && (flags & (ADSB_FLAG_FEC_SOFT | ADSB_FLAG_CONFIDENCE | ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE |
                                                      ADSB_FLAG_FRAMER_SLICES))) return -EINVAL;
  if ((flags & ADSB_FLAG_STREAM_DECODE_SHARED) && !(flags & ADSB_FLAG_STREAM_DECODE)) return -EINVAL;           // no decoder to share
  if ((flags & ADSB_FLAG_STREAM_DEDUP) && !(flags & ADSB_FLAG_STREAM_DECODE_SHARED)) return -EINVAL;             // one decoder, or nothing is heard twice
  if (!out) return -EINVAL;
  *out = nullptr;
  if (!(fs > 0) || fmod(fs, 1e6) != 0.0) return -EINVAL;        // framer.py:44, demod.py:42
  long long sps = (long long)(fs / 1e6);
  if (sps < 2 || (sps & 1) || sps > ADSB_MAX_SPS) return -EINVAL;   // odd sps crashes the reference's work(); above the maximum: untested
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -ENODEV;   // no CPU fallback, by design
  if (device < 0 || device >= ndev) return -ENODEV;
  adsb_ctx* c = new (std::nothrow) adsb_ctx();
  if (!c) return -ENOMEM;
  c->device = device; c->fs = fs; c->sps = (int)sps; c->thr = threshold; c->flags = flags;
  if (hipSetDevice(device) != hipSuccess) { delete c; return -ENODEV; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
  probe_numa(c);
  if (flags & ADSB_FLAG_NO_NUMA_BINDING) c->numa_node = -1;    // (the cpu list stays readable through adsb_numa_info)
  {
    int nb;
    if ((nb = detect_occupancy<0>(c->det_dyn_lds[0])) > 0) c->bpc[0] = nb;
    if ((nb = detect_occupancy<1>(c->det_dyn_lds[1])) > 0) c->bpc[1] = nb;
    if ((nb = detect_occupancy<2>(c->det_dyn_lds[2])) > 0) c->bpc[2] = nb;
    if ((nb = detect_occupancy<3>(c->det_dyn_lds[3])) > 0) c->bpc[3] = nb;
    if ((nb = detect_occupancy<4>(c->det_dyn_lds[4])) > 0) c->bpc[4] = nb;
    const unsigned st[ADSB_FMT_COUNT] = {detect_static_lds<0>(), detect_static_lds<1>(), detect_static_lds<2>(),
                                         detect_static_lds<3>(), detect_static_lds<4>()};
    for (int m = 0; m < ADSB_FMT_COUNT; ++m) {
      const unsigned per = (st[m] + c->det_dyn_lds[m] + 1279u) / 1280u * 1280u;             // LDS allocation granule on gfx950
      const unsigned used = per * (unsigned)c->bpc[m];
      c->lds_beside[m] = used < 163840u ? 163840u - used : 0u;
    }
  }
  c->own_stream = true;
  // submitted passes overlap on the slots' streams unless the caller opts out (ADSB_FLAG_SINGLE_STREAM: everything on ONE stream)
  c->split_tail = (flags & ADSB_FLAG_SINGLE_STREAM) == 0;
  for (Event& e : c->ring_done)
    if (hipEventCreateWithFlags(&e.p, hipEventDisableTiming) != hipSuccess) { adsb_destroy(c); return -EIO; }
  for (Slot& sl : c->slot) {
    if (host_alloc_near(c, (void**)&sl.h_sum.p, sizeof(Summary), true) != hipSuccess) { adsb_destroy(c); return -ENOMEM; }
    memset(sl.h_sum, 0, sizeof(Summary));                        // (pad_ is the pass number finish() polls: starts at zero)
    if (hipStreamCreateWithFlags(&sl.stream.p, hipStreamNonBlocking) != hipSuccess) { adsb_destroy(c); return -EIO; }
    if (hipEventCreate(&sl.ev0.p) != hipSuccess || hipEventCreate(&sl.ev1.p) != hipSuccess ||
        hipEventCreateWithFlags(&sl.done.p, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sl.det_done.p, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&sl.h2d_done.p, hipEventDisableTiming) != hipSuccess) { adsb_destroy(c); return -EIO; }
  }
  c->stream = c->slot[0].stream;         // blocking calls always run in slot 0 (run_pipeline)
  if (hipStreamCreateWithFlags(&c->h2d_stream.p, hipStreamNonBlocking) != hipSuccess) { adsb_destroy(c); return -EIO; }
  if (flags & ADSB_FLAG_DECODE) {
    // every entry's epoch 0: no plane; adsb_reset moves the epoch on
    const size_t pb = ((size_t)1 << 24) * sizeof(Plane);
    if (hipMalloc((void**)&c->d_planes.p, pb) != hipSuccess) { (void)hipGetLastError(); adsb_destroy(c); return -ENOMEM; }
    if (hipMemsetAsync(c->d_planes, 0, pb, c->stream) != hipSuccess) { adsb_destroy(c); return -EIO; }
    // last_seen: written by the fold that creates the plane, read only beside a live plane -- never cleared
    if ((flags & ADSB_FLAG_PLANE_AGES) && hipMalloc((void**)&c->d_seen.p, ((size_t)1 << 24) * sizeof(long long)) != hipSuccess) {
      (void)hipGetLastError(); adsb_destroy(c); return -ENOMEM;
    }
  }
  if (flags & ADSB_FLAG_AIRCRAFT_TABLE) {
    if (hipMalloc((void**)&c->d_air.p, ((size_t)1 << 24) * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&c->d_air_st.p, sizeof(AirState)) != hipSuccess) { (void)hipGetLastError(); adsb_destroy(c); return -ENOMEM; }
    if (hipEventCreateWithFlags(&c->air_ev.p, hipEventDisableTiming) != hipSuccess || air_clear(c) != 0) { adsb_destroy(c); return -EIO; }
  }
  *out = c;
  return 0;
}

// Nothing of the context is still at work on the device when its members let go of what they own.
void adsb_destroy(adsb_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (!c->own_stream && c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (c->h2d_stream) (void)hipStreamSynchronize(c->h2d_stream);
  if (c->d2h_stream) (void)hipStreamSynchronize(c->d2h_stream);
  if (c->tail_stream) (void)hipStreamSynchronize(c->tail_stream);
  for (Slot& sl : c->slot) if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  if (c->air_ev) (void)hipEventSynchronize(c->air_ev);
  delete c;
}

int adsb_set_threshold(adsb_ctx* c, float threshold) {
  if (!c) return -EINVAL;
  c->thr = threshold;
  return 0;
}

int adsb_set_stream(adsb_ctx* c, void* hip_stream) {
  if (!c) return -EINVAL;
  { int r = require_idle(c, "calls pending"); if (r) return r; }
  if (c->own_stream && c->stream) (void)hipStreamSynchronize(c->stream);      // (slot 0's: it stays the slot's)
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream.p, hipStreamNonBlocking));
  if (!c->tail_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->tail_stream.p, hipStreamNonBlocking));
  c->stream = (hipStream_t)hip_stream;
  c->own_stream = false;
  return 0;
}

int adsb_set_copy_threads(adsb_ctx* c, int32_t threads) {
  if (!c || threads < 1 || threads > 64) return -EINVAL;
  if (c->pool) return fail(c, -EBUSY, "copy threads already running (set before the first pageable submission)");
  c->copy_threads = threads - 1;                            // the calling thread is one of them
  return 0;
}

int adsb_numa_info(adsb_ctx* c, int32_t* node, char* cpulist, size_t cap, char* pci_bdf, size_t bdf_cap) {
  if (!c) return -EINVAL;
  if (node) *node = c->numa_node;
  if (cpulist && cap) snprintf(cpulist, cap, "%s", c->cpulist);
  if (pci_bdf && bdf_cap) snprintf(pci_bdf, bdf_cap, "%s", c->pci_bdf);
  return 0;
}

int adsb_host_alloc_near(adsb_ctx* c, void** p, size_t bytes) {
  if (!c || !p || bytes == 0) return -EINVAL;
  *p = nullptr;
  return host_alloc_near(c, p, bytes) == hipSuccess ? 0 : -ENOMEM;
}

int adsb_host_copy(adsb_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c || (bytes > 0 && (!dst || !src))) return -EINVAL;
  int rc = ensure_pool(c);
  if (rc) return rc;
  c->pool->copy((char*)dst, (const char*)src, bytes);
  return 0;
}

int adsb_wait_for_event(adsb_ctx* c, void* hip_event) {
  if (!c || !hip_event) return -EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  // The NEXT call -- blocking, submitted or host-fed -- runs after the event: the wait is queued with that call, on the stream
  // its first operation runs on (which one is decided there; a host-fed submission: the upload stream).  Nothing is queued
  // now: a stream that is never used never takes one of the process's four hardware queues.  The event has to stay alive
  // until that call; a later submission that depends on the same producer asks again (FrontEnd does, per tensor call).
  if (c->n_ext == adsb_ctx::kMaxExt) {           // more producers than remembered: the oldest is waited for by every queue now
    for (Slot& sl : c->slot) HIPCHK(c, hipStreamWaitEvent(sl.stream, c->ext_ev[0], 0));
    if (!c->own_stream) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ext_ev[0], 0));
    HIPCHK(c, hipStreamWaitEvent(c->h2d_stream, c->ext_ev[0], 0));
    for (int i = 1; i < c->n_ext; ++i) c->ext_ev[i - 1] = c->ext_ev[i];
    --c->n_ext;
  }
  c->ext_ev[c->n_ext++] = (hipEvent_t)hip_event;
  return 0;
}

int adsb_clear_pending_events(adsb_ctx* c) {
  if (!c) return -EINVAL;
  c->n_ext = 0;
  return 0;
}

int adsb_reset(adsb_ctx* c) {
  if (!c) return -EINVAL;
  if (c->flags & ADSB_FLAG_AIRCRAFT_TABLE) {
    int r = require_idle(c, kCallPending);
    if (r) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if ((c->flags & ADSB_FLAG_DECODE) && ++c->dec_epoch == 0) {   // (2^32 resets: every entry cleared once more, behind
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->air_ev, 0));    //  every step queued so far and before air_clear's event)
      HIPCHK(c, hipMemsetAsync(c->d_planes, 0, ((size_t)1 << 24) * sizeof(Plane), c->stream));
      c->dec_epoch = 1;
    }
    if ((r = air_clear(c))) return r;
  }
  c->st = FramerState();
  c->n_ext = 0;           // a fresh stream starts without remembered producers
  for (StreamState& s : c->sb.st) stream_make_fresh(s);
  if (c->fd.open) {
    for (size_t s = 0; s < c->fd.gen.size(); ++s) { const int r = fleet_reset_stream(c, s); if (r) return r; }
    c->fd.call = 0;          // (no slot of an earlier generation is looked up again)
  }
  return 0;
}

int adsb_framer_state(adsb_ctx* c, float* prev_in0, int64_t* prev_eob_idx) {
  if (!c) return -EINVAL;
  if (prev_in0) *prev_in0 = c->st.prev_in0;
  if (prev_eob_idx) *prev_eob_idx = (int64_t)c->st.prev_eob;
  return 0;
}

// The entry points named after one format are the format-generic ones with that format.
int adsb_set_iq16_scale(adsb_ctx* c, float scale) { return adsb_set_format_scale(c, ADSB_FMT_SC16, scale); }
int adsb_process_iq(adsb_ctx* c, const float* iq_host, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format(c, ADSB_FMT_FC32, iq_host, n, abs_offset, out, cap, n_out);
}
int adsb_process_iq_device(adsb_ctx* c, const void* d_iq, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format_device(c, ADSB_FMT_FC32, d_iq, n, abs_offset, out, cap, n_out);
}
int adsb_submit_iq_device(adsb_ctx* c, const void* d_iq, int64_t n, int64_t abs_offset, int32_t* ticket) {
  return adsb_submit_format_device(c, ADSB_FMT_FC32, d_iq, n, abs_offset, ticket);
}
int adsb_process_mag2(adsb_ctx* c, const float* mag2_host, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format(c, ADSB_FMT_MAG2, mag2_host, n, abs_offset, out, cap, n_out);
}
int adsb_process_mag2_device(adsb_ctx* c, const void* d_mag2, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format_device(c, ADSB_FMT_MAG2, d_mag2, n, abs_offset, out, cap, n_out);
}
int adsb_submit_mag2_device(adsb_ctx* c, const void* d_mag2, int64_t n, int64_t abs_offset, int32_t* ticket) {
  return adsb_submit_format_device(c, ADSB_FMT_MAG2, d_mag2, n, abs_offset, ticket);
}
int adsb_process_iq16(adsb_ctx* c, const int16_t* iq16_host, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format(c, ADSB_FMT_SC16, iq16_host, n, abs_offset, out, cap, n_out);
}
int adsb_process_iq16_device(adsb_ctx* c, const void* d_iq16, int64_t n, int64_t abs_offset, adsb_burst* out, int32_t cap, int32_t* n_out) {
  return adsb_process_format_device(c, ADSB_FMT_SC16, d_iq16, n, abs_offset, out, cap, n_out);
}
int adsb_submit_iq16_device(adsb_ctx* c, const void* d_iq16, int64_t n, int64_t abs_offset, int32_t* ticket) {
  return adsb_submit_format_device(c, ADSB_FMT_SC16, d_iq16, n, abs_offset, ticket);
}

int adsb_set_format_scale(adsb_ctx* c, int format, float scale) {
  if (!c || format < ADSB_FMT_SC16 || format >= ADSB_FMT_COUNT) return -EINVAL;
  c->scale[format] = scale;
  return 0;
}

int adsb_process_format_device(adsb_ctx* c, int format, const void* d_data, int64_t n, int64_t abs_offset,
                               adsb_burst* out, int32_t cap, int32_t* n_out) {
  if (!c || format < 0 || format >= ADSB_FMT_COUNT) return -EINVAL;
  return canonical(c, format, d_data, n, abs_offset, out, cap, n_out);
}

int adsb_process_format(adsb_ctx* c, int format, const void* host, int64_t n, int64_t abs_offset, adsb_burst* out,
                        int32_t cap, int32_t* n_out) {
  if (!c || format < 0 || format >= ADSB_FMT_COUNT || n < 0 || (n > 0 && !host)) return -EINVAL;
  if (n == 0) { if (n_out) *n_out = 0; c->slot[c->last_slot].nres = 0; return 0; }
  HIPCHK(c, hipSetDevice(c->device));
  void* d = nullptr;
  int rc = upload(c, host, (size_t)n * (size_t)mode_bytes(format), &d);
  if (rc) return rc;
  return canonical(c, format, d, n, abs_offset, out, cap, n_out);
}

static_assert(sizeof(adsb_batch_item) == 32 && offsetof(adsb_batch_item, threshold) == 24, "adsb_batch_item layout");
static_assert(ADSB_BATCH_ITEM_MAX == kBatchItemMax, "adsb_plan.h and the header agree on the longest batch-path item");

int adsb_process_batch_device(adsb_ctx* c, int format, const adsb_batch_item* items, int32_t n_items, adsb_burst* out,
                              int32_t cap, int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  int rc = check_batch(c, format, items, n_items, out, cap, item_first, n_out);
  if (rc) return rc;
  return run_batch(c, format, items, n_items, out, cap, item_first, n_out, n_fallback);
}

static_assert(sizeof(adsb_stream_item) == 32 && offsetof(adsb_stream_item, stream) == 16 && offsetof(adsb_stream_item, threshold) == 24,
              "adsb_stream_item layout");

int adsb_streams_open(adsb_ctx* c, int32_t n_streams) {
  if (!c) return -EINVAL;
  if (n_streams < 1) return fail(c, -EINVAL, "adsb_streams_open: n_streams < 1");
  if (c->flags & (ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE | ADSB_FLAG_CONFIDENCE))
    return fail(c, -EINVAL, "adsb_streams_open: not for ADSB_FLAG_AIRCRAFT_TABLE / _DECODE / _CONFIDENCE contexts (one receiver each)");
  if (c->flags & ADSB_FLAG_FEC_SOFT) return fail(c, -EINVAL, "adsb_streams_open: not for ADSB_FLAG_FEC_SOFT contexts");
  int rc = require_idle(c, kCallPending);
  if (rc) return rc;
  if (!c->sb.st.empty()) return fail(c, -EINVAL, "adsb_streams_open: streams are open (adsb_streams_close first)");
  HIPCHK(c, hipSetDevice(c->device));
  StreamBufs& S = c->sb;
  S.slot_bytes = ((size_t)stream_carry_max(c->sps) * 8 + 255) & ~(size_t)255;
  if ((c->flags & ADSB_FLAG_STREAM_DECODE) && n_streams > (1 << kFleetStreamBits))
    return fail(c, -EINVAL, "adsb_streams_open: at most 2^20 streams with ADSB_FLAG_STREAM_DECODE");
  if ((rc = ensure(c, S.d_carry, (size_t)n_streams * 2 * S.slot_bytes))) return rc;
  if ((c->flags & ADSB_FLAG_STREAM_DECODE) && (rc = fleet_open(c, (size_t)n_streams))) return rc;
  S.st.assign((size_t)n_streams, StreamState());
  return 0;
}

int adsb_streams_close(adsb_ctx* c) {
  if (!c) return -EINVAL;
  int rc = require_idle(c, kCallPending);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  StreamBufs& S = c->sb;
  S.st.clear();
  S.slot_bytes = 0;
  for (DevBuf* b : {&S.d_carry, &S.d_stage, &S.d_tab}) HIPCHK(c, b->release());
  for (PinnedBuf* b : {&S.h_tab, &S.h_status}) HIPCHK(c, b->release());
  if (c->fd.open) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return fleet_close(c);
  }
  return 0;
}

int adsb_stream_set_base(adsb_ctx* c, int32_t stream, int64_t abs_offset) {
  if (!c) return -EINVAL;
  if (stream < 0 || (size_t)stream >= c->sb.st.size()) return fail(c, -EINVAL, "adsb_stream_set_base: no such stream");
  if (c->sb.st[(size_t)stream].pos != 0) return fail(c, -EINVAL, "adsb_stream_set_base: the stream is not fresh");
  c->sb.st[(size_t)stream].base = abs_offset;
  return 0;
}

int adsb_stream_state(adsb_ctx* c, int32_t stream, int64_t* pos, int64_t* eob, int64_t* n_overlong) {
  if (!c) return -EINVAL;
  if (stream < 0 || (size_t)stream >= c->sb.st.size()) return fail(c, -EINVAL, "adsb_stream_state: no such stream");
  const StreamState& s = c->sb.st[(size_t)stream];
  if (pos) *pos = s.pos;
  if (eob) *eob = s.eob;
  if (n_overlong) *n_overlong = s.overlong;
  return 0;
}

int adsb_stream_reset(adsb_ctx* c, int32_t stream) {
  if (!c) return -EINVAL;
  if (stream < 0 || (size_t)stream >= c->sb.st.size()) return fail(c, -EINVAL, "adsb_stream_reset: no such stream");
  stream_make_fresh(c->sb.st[(size_t)stream]);
  if (c->fd.open && !(c->flags & ADSB_FLAG_STREAM_DECODE_SHARED)) return fleet_reset_stream(c, (size_t)stream);
  return 0;               // (a shared decoder is nobody's: adsb_streams_decoder_reset)
}

// 0 when the context was created with `flag` and has open streams, else -EINVAL with the entry point's (`api`) message
static int need_streams(adsb_ctx* c, uint32_t flag, const char* flag_name, const char* api) {
  char msg[160];
  if (!(c->flags & flag)) {
    snprintf(msg, sizeof(msg), "context created without %s", flag_name);
    return fail(c, -EINVAL, msg);
  }
  if (!c->fd.open) {
    snprintf(msg, sizeof(msg), "%s: no streams (adsb_streams_open first)", api);
    return fail(c, -EINVAL, msg);
  }
  return 0;
}
static int need_shared_streams(adsb_ctx* c, const char* api) { return need_streams(c, ADSB_FLAG_STREAM_DECODE_SHARED, "ADSB_FLAG_STREAM_DECODE_SHARED", api); }
static int need_dedup_streams(adsb_ctx* c, const char* api) { return need_streams(c, ADSB_FLAG_STREAM_DEDUP, "ADSB_FLAG_STREAM_DEDUP", api); }

int adsb_streams_decoder_reset(adsb_ctx* c) {
  if (!c) return -EINVAL;
  if (const int rc = need_shared_streams(c, "adsb_streams_decoder_reset")) return rc;
  return fleet_reset_stream(c, 0);
}

int adsb_stream_last_order(adsb_ctx* c, const int32_t** order, int32_t* n) {
  if (!c) return -EINVAL;
  if (const int rc = need_shared_streams(c, "adsb_stream_last_order")) return rc;
  if (order) *order = c->fd.n_rows > 0 ? (const int32_t*)c->fd.h_order.p : nullptr;
  if (n) *n = c->fd.n_rows;
  return 0;
}

int adsb_streams_set_dedup(adsb_ctx* c, double window_s, double horizon_s) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_streams_set_dedup")) return rc;
  if (!(window_s >= 0) || !(horizon_s >= window_s)) return fail(c, -EINVAL, "adsb_streams_set_dedup: 0 <= window_s <= horizon_s, no NaN");
  if (c->fd.dd.delivered) return fail(c, -EINVAL, "adsb_streams_set_dedup: a call has been delivered since the decoder was fresh");
  c->fd.dd.window = window_s; c->fd.dd.horizon = horizon_s;
  return 0;
}

int adsb_stream_last_duplicates(adsb_ctx* c, const int32_t** dup, int32_t* n) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_last_duplicates")) return rc;
  if (dup) *dup = c->fd.n_rows > 0 ? (const int32_t*)c->fd.dd.h_dup.p : nullptr;
  if (n) *n = c->fd.n_rows;
  return 0;
}

int adsb_stream_dedup_stats(adsb_ctx* c, int64_t* duplicates, int64_t* carried, double* hi) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_dedup_stats")) return rc;
  if (duplicates) *duplicates = c->fd.dd.duplicates;
  if (carried) *carried = c->fd.dd.cnt;
  if (hi) *hi = c->fd.dd.hi;
  return 0;
}

int adsb_stream_set_ecef(adsb_ctx* c, int32_t stream, double x, double y, double z) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_set_ecef")) return rc;
  if (stream < 0 || (size_t)stream >= c->fd.rx.size() / 3) return fail(c, -EINVAL, "adsb_stream_set_ecef: no such stream");
  if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return fail(c, -EINVAL, "adsb_stream_set_ecef: a position is three finite numbers");
  double* const r = &c->fd.rx[3 * (size_t)stream];
  r[0] = x; r[1] = y; r[2] = z;
  return 0;
}

int adsb_stream_mlat_stats(adsb_ctx* c, int32_t* positioned, double* ts_ulp_m) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_mlat_stats")) return rc;
  if (positioned) {
    int32_t k = 0;
    for (size_t s = 0; s < c->fd.rx.size(); s += 3) k += !std::isnan(c->fd.rx[s]);
    *positioned = k;
  }
  if (ts_ulp_m) {
    const double hi = std::fabs(c->fd.dd.hi);
    *ts_ulp_m = ADSB_MLAT_C * (std::nextafter(hi, std::numeric_limits<double>::infinity()) - hi);
  }
  return 0;
}

static_assert(sizeof(adsb_mlat_aux) == adsb_mlat_host::kAuxBytes && sizeof(adsb_mlat_rule) == 24 && offsetof(adsb_mlat_aux, alt_ft) == 16 &&
              offsetof(adsb_mlat_aux, flags) == 24, "adsb_mlat_rule.hip writes adsb_mlat_aux rows");

// One multilateration call, behind the argument table of the entry point `api` (whose name its messages carry): the three
// phases on the carry as it stands; the head count, then the group and member counts, come down between them (as
// fleet_step's h_cnt); -ENOSPC is decided before the solve.  The work buffer is sized from the carry's length before the first
// launch.  rule null: adsb_mlat.hip's groups and Gauss-Newton kernels on layout().  rule given: adsb_mlat_rule.hip's groups and
// damped solve kernels on layout_rule(), the aux rows (aux may be null) beside the fixes.  min_group: the fewest used
// hearings a selected group can have, which bounds the group count.
// mlat_solve is the call up to and including the solve's launch: the fixes, the aux rows and the member lists are left in
// F.d_mlat, carved by *L_out, for mlat_call to bring down or for adsb_stream_mlat_track to read where they lie.
static int mlat_solve(adsb_ctx* c, const char* api, double t_lo, double t_hi, int32_t min_rx, int min_group, const adsb_mlat_rule* rule, int32_t cap,
                      int32_t* n_fixes, int32_t member_cap, int32_t* n_members, adsb_mlat_host::Layout* L_out) {
  namespace mh = adsb_mlat_host;
  const auto refuse = [&](int code, const char* what, hipError_t he = hipSuccess) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", api, what);
    return fail(c, code, msg, he);
  };
  int rc;
  if ((rc = require_idle(c, kCallPending))) return rc;
  FleetDec& F = c->fd;
  const FleetDec::Dedup& D = F.dd;
  *n_fixes = 0; *n_members = 0;
  const int nc = D.cnt, n_streams = (int)(F.rx.size() / 3);
  if (nc == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = c->stream;
  const mh::Layout L = rule ? mh::layout_rule((size_t)nc, (size_t)n_streams) : mh::layout((size_t)nc, (size_t)n_streams);
  *L_out = L;
  const size_t rx_bytes = F.rx.size() * sizeof(double);
  if ((rc = ensure(c, F.d_mlat, L.bytes)) || (rc = ensure_pinned(c, F.h_mlat, rx_bytes + 64))) return rc;
  char* const work = (char*)F.d_mlat.p;
  int* const got = (int*)((char*)F.h_mlat.p + rx_bytes);
  memcpy(F.h_mlat.p, F.rx.data(), rx_bytes);
  HIPCHK(c, hipMemcpyAsync(work + L.rx, F.h_mlat.p, rx_bytes, hipMemcpyHostToDevice, st));
  const char* const carry = (const char*)D.d_carry[D.cur].p + (size_t)D.off * adsb_dedup_host::kEntBytes;
  hipError_t e;
  if ((e = (hipError_t)mh::launch_heads(st, carry, nc, t_lo, t_hi, D.window, work, L))) return refuse(-EIO, "the head kernels", e);
  HIPCHK(c, hipMemcpyAsync(got, work + L.tot_heads, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int nh = got[1];
  if (nh < 0 || nh > nc) return refuse(-EIO, "the head count is out of range");
  if (nh == 0) return 0;
  if ((e = (hipError_t)(rule ? mh::launch_groups_rule : mh::launch_groups)(st, carry, nc, nh, D.window, min_rx, n_streams, work, L)))
    return refuse(-EIO, "the group kernels", e);
  HIPCHK(c, hipMemcpyAsync(got, work + L.tot_groups, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int ng = got[1], nm = got[2];
  if (ng < 0 || ng > nc / min_group || nm < (long long)ng * min_rx || nm > nc) return refuse(-EIO, "the group counts are out of range");
  *n_fixes = ng; *n_members = nm;
  if (ng > cap || nm > member_cap) return refuse(-ENOSPC, "cap or member_cap is too small (*n_fixes, *n_members)");
  if (ng == 0) return 0;
  if (rule) {
    const double alt_weight = (rule->flags & ADSB_MLAT_ALTITUDE) ? rule->alt_weight : 0.0;
    if ((e = (hipError_t)mh::launch_solve_lm(st, carry, nc, ng, D.window, n_streams, rule->flags, alt_weight, work, L))) return refuse(-EIO, "k_mlat_solve_lm", e);
  } else if ((e = (hipError_t)mh::launch_solve(st, carry, nc, ng, D.window, n_streams, work, L))) {
    return refuse(-EIO, "k_mlat_solve", e);
  }
  return 0;
}

static int mlat_call(adsb_ctx* c, const char* api, double t_lo, double t_hi, int32_t min_rx, int min_group, const adsb_mlat_rule* rule,
                     adsb_mlat_fix* fixes, adsb_mlat_aux* aux, int32_t cap, int32_t* n_fixes, int32_t* member_stream, double* member_ts,
                     int32_t member_cap, int32_t* n_members) {
  char msg[192];
  if (std::isnan(t_lo) || std::isnan(t_hi)) { snprintf(msg, sizeof(msg), "%s: a bound is NaN", api); return fail(c, -EINVAL, msg); }
  if (!n_fixes || !n_members || cap < 0 || member_cap < 0 || (cap > 0 && !fixes) || (member_cap > 0 && (!member_stream || !member_ts))) {
    snprintf(msg, sizeof(msg), "%s: n_fixes / n_members, or the arrays for cap / member_cap > 0, missing", api);
    return fail(c, -EINVAL, msg);
  }
  adsb_mlat_host::Layout L;
  if (const int rc = mlat_solve(c, api, t_lo, t_hi, min_rx, min_group, rule, cap, n_fixes, member_cap, n_members, &L)) return rc;
  const int ng = *n_fixes, nm = *n_members;
  if (ng == 0) return 0;
  const hipStream_t st = c->stream;
  const char* const work = (const char*)c->fd.d_mlat.p;
  HIPCHK(c, hipMemcpyAsync(fixes, work + L.fixes, (size_t)ng * sizeof(adsb_mlat_fix), hipMemcpyDeviceToHost, st));
  if (rule && aux) HIPCHK(c, hipMemcpyAsync(aux, work + L.aux, (size_t)ng * sizeof(adsb_mlat_aux), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(member_stream, work + L.member_stream, (size_t)nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(member_ts, work + L.member_ts, (size_t)nm * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

int adsb_stream_mlat(adsb_ctx* c, double t_lo, double t_hi, int32_t min_rx, adsb_mlat_fix* fixes, int32_t cap, int32_t* n_fixes,
                     int32_t* member_stream, double* member_ts, int32_t member_cap, int32_t* n_members) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_mlat")) return rc;
  if (min_rx < adsb_mlat_host::kMinRx) return fail(c, -EINVAL, "adsb_stream_mlat: min_rx < 4 (three-receiver fixes are not provided)");
  return mlat_call(c, "adsb_stream_mlat", t_lo, t_hi, min_rx, adsb_mlat_host::kMinRx, nullptr, fixes, nullptr, cap, n_fixes, member_stream, member_ts,
                   member_cap, n_members);
}

// adsb_mlat_rule's argument table, for the entry point `api`: 0, or -EINVAL with its message
static int mlat_rule_check(adsb_ctx* c, const char* api, const adsb_mlat_rule* rule) {
  const auto refuse = [&](const char* what) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", api, what);
    return fail(c, -EINVAL, msg);
  };
  if (!rule) return refuse("rule is NULL");
  if (rule->solver != ADSB_MLAT_SOLVER_GN && rule->solver != ADSB_MLAT_SOLVER_LM) return refuse("unknown solver");
  if (rule->flags & ~(ADSB_MLAT_RESTART | ADSB_MLAT_ALTITUDE)) return refuse("unknown flags");
  if (rule->solver == ADSB_MLAT_SOLVER_GN && rule->flags != 0) return refuse("flags need ADSB_MLAT_SOLVER_LM");
  if (rule->reserved != 0) return refuse("reserved is not 0");
  const bool want_alt = (rule->flags & ADSB_MLAT_ALTITUDE) != 0;
  if (rule->min_rx < (want_alt ? adsb_mlat_host::kMinRxAided : adsb_mlat_host::kMinRx)) return refuse("min_rx < 4 (< 3 with ADSB_MLAT_ALTITUDE)");
  if (want_alt && !(std::isfinite(rule->alt_weight) && rule->alt_weight > 0.0)) return refuse("alt_weight is not finite and > 0");
  return 0;
}

// adsb_stream_mlat with the rule stated by the caller.  _GN is adsb_stream_mlat itself, with empty aux rows; _LM is
// mlat_call with the rule.
int adsb_stream_mlat_rule(adsb_ctx* c, double t_lo, double t_hi, const adsb_mlat_rule* rule, adsb_mlat_fix* fixes, adsb_mlat_aux* aux, int32_t cap,
                          int32_t* n_fixes, int32_t* member_stream, double* member_ts, int32_t member_cap, int32_t* n_members) {
  if (!c) return -EINVAL;
  if (const int rc = need_dedup_streams(c, "adsb_stream_mlat_rule")) return rc;
  if (const int rc = mlat_rule_check(c, "adsb_stream_mlat_rule", rule)) return rc;
  if (rule->solver == ADSB_MLAT_SOLVER_GN) {
    const int rc = adsb_stream_mlat(c, t_lo, t_hi, rule->min_rx, fixes, cap, n_fixes, member_stream, member_ts, member_cap, n_members);
    if (rc == 0 && aux)
      for (int32_t k = 0; k < *n_fixes; ++k) { memset(&aux[k], 0, sizeof aux[k]); aux[k].alt_ft = -1; }
    return rc;
  }
  return mlat_call(c, "adsb_stream_mlat_rule", t_lo, t_hi, rule->min_rx, adsb_mlat_host::kMinRxAided, rule, fixes, aux, cap, n_fixes, member_stream,
                   member_ts, member_cap, n_members);
}

// ---- MLAT TRACKS (include/adsb_hip.h): the store of FleetDec::Tracks, adsb_mlat_track.hip's kernels
static_assert(sizeof(adsb_mlat_track) == adsb_mlat_track_host::kRowBytes && sizeof(adsb_mlat_track_rule) == adsb_mlat_track_host::kRuleBytes &&
              sizeof(adsb_mlat_track_stats) == 64 && offsetof(adsb_mlat_track, first_ts) == 16 && offsetof(adsb_mlat_track, n_rx) == 88 &&
              offsetof(adsb_mlat_track_rule, restart_after) == 56 && sizeof(adsb_mlat_fix) == adsb_mlat_track_host::kFixBytes &&
              sizeof(adsb_mlat_aux) == adsb_mlat_track_host::kAuxBytes && ADSB_MLAT_OK == 0,
              "adsb_mlat_track.hip reads adsb_mlat_fix and adsb_mlat_aux rows and writes adsb_mlat_track rows");

// One update of the track store: the rule's argument tables, mlat_solve -- the fixes and aux rows stay in F.d_mlat -- then
// adsb_mlat_track.hip's two launch groups.  The eligible count comes down between them (the sort's size is the host's); the other
// buffer is given room for every eligible fix to start a track before the launch that merges into it; the run and
// new-address counts and the totals come down behind it, and only then do cur and n change.
int adsb_stream_mlat_track(adsb_ctx* c, double t_lo, double t_hi, const adsb_mlat_rule* rule, const adsb_mlat_track_rule* tr,
                           adsb_mlat_track_stats* stats) {
  namespace mt = adsb_mlat_track_host;
  const char* const api = "adsb_stream_mlat_track";
  if (!c) return -EINVAL;
  int rc;
  if ((rc = need_dedup_streams(c, api)) || (rc = mlat_rule_check(c, api, rule))) return rc;
  const auto refuse = [&](int code, const char* what, hipError_t he = hipSuccess) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", api, what);
    return fail(c, code, msg, he);
  };
  if (!tr) return refuse(-EINVAL, "track_rule is NULL");
  const auto gain = [](double v) { return std::isfinite(v) && v > 0.0 && v <= 1.0; };
  const auto bound = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (!gain(tr->alpha) || !gain(tr->beta)) return refuse(-EINVAL, "alpha and beta are finite and in (0, 1]");
  if (!bound(tr->gate_m) || !bound(tr->max_speed_mps) || !bound(tr->max_gap_s)) return refuse(-EINVAL, "gate_m, max_speed_mps and max_gap_s are finite and >= 0");
  if (std::isnan(tr->max_rms_m) || std::isnan(tr->min_up_m)) return refuse(-EINVAL, "max_rms_m or min_up_m is NaN");
  if (tr->restart_after < 1) return refuse(-EINVAL, "restart_after < 1");
  if (tr->reserved != 0) return refuse(-EINVAL, "track_rule->reserved is not 0");
  if (std::isnan(t_lo) || std::isnan(t_hi)) return refuse(-EINVAL, "a bound is NaN");
  FleetDec& F = c->fd;
  FleetDec::Tracks& T = F.trk;
  adsb_mlat_track_stats s = {};
  s.tracks = T.n;
  const bool lm = rule->solver == ADSB_MLAT_SOLVER_LM;
  adsb_mlat_host::Layout ML;
  int32_t ng = 0, nm = 0;
  if ((rc = mlat_solve(c, api, t_lo, t_hi, rule->min_rx, lm ? adsb_mlat_host::kMinRxAided : adsb_mlat_host::kMinRx, lm ? rule : nullptr, INT32_MAX, &ng,
                       INT32_MAX, &nm, &ML)))
    return rc;
  s.fixes = ng;
  if (ng > 0) {
    const hipStream_t st = c->stream;
    const char* const fixes = (const char*)F.d_mlat.p + ML.fixes;
    const char* const aux = lm ? (const char*)F.d_mlat.p + ML.aux : nullptr;
    const mt::Layout L = mt::layout((size_t)ng);
    if ((rc = ensure(c, T.d_work, L.bytes)) || (rc = ensure_pinned(c, T.h_cnt, 256))) return rc;
    char* const work = (char*)T.d_work.p;
    int* const cnts = (int*)T.h_cnt.p;
    const unsigned long long* const tot = (const unsigned long long*)((char*)T.h_cnt.p + 128);
    hipError_t e;
    if ((e = (hipError_t)mt::launch_keys(st, fixes, ng, work, L))) return refuse(-EIO, "the key kernels", e);
    HIPCHK(c, hipMemcpyAsync(cnts, work + L.cnts, mt::kCntWords * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int nk = cnts[mt::kCntKeys];
    if (nk < 0 || nk > ng) return refuse(-EIO, "the eligible count is out of range");
    s.eligible = nk;
    if (nk > 0) {
      if ((long long)T.n + nk > (1ll << 24)) return refuse(-EIO, "more tracks than addresses");
      DevBuf& next = T.d_rows[T.cur ^ 1];
      if ((rc = ensure(c, next, ((size_t)T.n + (size_t)nk) * mt::kRowBytes))) return rc;
      if ((e = (hipError_t)mt::launch_update(st, fixes, aux, nk, tr, T.d_rows[T.cur].p, T.n, next.p, work, L))) return refuse(-EIO, "the update kernels", e);
      HIPCHK(c, hipMemcpyAsync(cnts, work + L.cnts, mt::kCntWords * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync((char*)T.h_cnt.p + 128, work + L.stats, mt::kStatWords * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      const int nr = cnts[mt::kCntRuns], nn = cnts[mt::kCntNew];
      if (nr < 1 || nr > nk || nn < 0 || nn > nr) return refuse(-EIO, "the run counts are out of range");
      T.cur ^= 1; T.n += nn;
      s.unusable = (int64_t)tot[mt::kStatUnusable]; s.stale = (int64_t)tot[mt::kStatStale]; s.rejected = (int64_t)tot[mt::kStatRejected];
      s.taken = (int64_t)tot[mt::kStatTaken]; s.started = (int64_t)tot[mt::kStatStarted];
      s.tracks = T.n;
    }
  }
  if (stats) *stats = s;
  return 0;
}

// The readout and the expiry: the predicate and the compaction over the store, the picked rows gathered into the other
// buffer, where the readout downloads them and which the expiry makes the store.  expire: no cap applies, and nothing is
// gathered when every row is kept.  -> *picked
static int tracks_pick(adsb_ctx* c, const char* api, int32_t min_fixes, double cutoff, int32_t cap, bool expire, int32_t* picked) {
  namespace mt = adsb_mlat_track_host;
  FleetDec::Tracks& T = c->fd.trk;
  const auto refuse = [&](int code, const char* what, hipError_t he = hipSuccess) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", api, what);
    return fail(c, code, msg, he);
  };
  *picked = 0;
  if (T.n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = c->stream;
  const mt::Layout L = mt::layout((size_t)T.n);
  int rc;
  DevBuf& next = T.d_rows[T.cur ^ 1];
  if ((rc = ensure(c, T.d_work, L.bytes)) || (rc = ensure_pinned(c, T.h_cnt, 256)) || (rc = ensure(c, next, (size_t)T.n * mt::kRowBytes))) return rc;
  char* const work = (char*)T.d_work.p;
  int* const cnts = (int*)T.h_cnt.p;
  hipError_t e;
  if ((e = (hipError_t)mt::launch_pick(st, T.d_rows[T.cur].p, T.n, min_fixes, cutoff, work, L))) return refuse(-EIO, "the pick kernels", e);
  HIPCHK(c, hipMemcpyAsync(cnts, work + L.cnts, mt::kCntWords * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int k = cnts[mt::kCntKeys];
  if (k < 0 || k > T.n) return refuse(-EIO, "the track count is out of range");
  *picked = k;
  if (!expire && k > cap) return refuse(-ENOSPC, "cap is too small (*n)");
  if (k == 0 || (expire && k == T.n)) return 0;
  if ((e = (hipError_t)mt::launch_gather(st, T.d_rows[T.cur].p, k, next.p, work, L))) return refuse(-EIO, "k_track_gather", e);
  return 0;
}

int adsb_stream_mlat_tracks(adsb_ctx* c, int32_t min_fixes, double cutoff, adsb_mlat_track* rows, int32_t cap, int32_t* n) {
  const char* const api = "adsb_stream_mlat_tracks";
  if (!c) return -EINVAL;
  int rc;
  if ((rc = need_dedup_streams(c, api))) return rc;
  if (!n || cap < 0 || (cap > 0 && !rows)) return fail(c, -EINVAL, "adsb_stream_mlat_tracks: n, or rows for cap > 0, missing");
  if (std::isnan(cutoff)) return fail(c, -EINVAL, "adsb_stream_mlat_tracks: cutoff is NaN");
  if ((rc = require_idle(c, kCallPending))) return rc;
  if ((rc = tracks_pick(c, api, min_fixes, cutoff, cap, false, n)) || *n == 0) return rc;
  FleetDec::Tracks& T = c->fd.trk;
  HIPCHK(c, hipMemcpyAsync(rows, T.d_rows[T.cur ^ 1].p, (size_t)*n * sizeof(adsb_mlat_track), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int adsb_stream_mlat_tracks_expire(adsb_ctx* c, double cutoff, int64_t* n_removed) {
  const char* const api = "adsb_stream_mlat_tracks_expire";
  if (!c) return -EINVAL;
  int rc;
  if ((rc = need_dedup_streams(c, api))) return rc;
  if (std::isnan(cutoff)) return fail(c, -EINVAL, "adsb_stream_mlat_tracks_expire: cutoff is NaN");
  if ((rc = require_idle(c, kCallPending))) return rc;
  if (n_removed) *n_removed = 0;
  FleetDec::Tracks& T = c->fd.trk;
  int32_t kept = 0;
  if ((rc = tracks_pick(c, api, INT32_MIN, cutoff, 0, true, &kept))) return rc;
  if (kept == T.n) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_removed) *n_removed = T.n - kept;
  T.cur ^= 1; T.n = kept;
  return 0;
}

int adsb_stream_mlat_tracks_reset(adsb_ctx* c) {
  if (!c) return -EINVAL;
  int rc;
  if ((rc = need_dedup_streams(c, "adsb_stream_mlat_tracks_reset")) || (rc = require_idle(c, kCallPending))) return rc;
  c->fd.trk.n = 0;
  return 0;
}

int adsb_streams_set_decoder(adsb_ctx* c, int32_t msg_filter) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (!c->fd.open) return fail(c, -EINVAL, "adsb_streams_set_decoder: no streams (adsb_streams_open first)");
  if (msg_filter != ADSB_DEC_ALL_MESSAGES && msg_filter != ADSB_DEC_EXTENDED_SQUITTER_ONLY) return fail(c, -EINVAL, "msg_filter");
  c->fd.all = msg_filter == ADSB_DEC_ALL_MESSAGES;
  return 0;
}

int adsb_stream_set_start(adsb_ctx* c, int32_t stream, double start_timestamp) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (stream < 0 || (size_t)stream >= c->fd.start.size()) return fail(c, -EINVAL, "adsb_stream_set_start: no such stream");
  if (c->sb.st[(size_t)stream].pos != 0) return fail(c, -EINVAL, "adsb_stream_set_start: the stream is not fresh");
  c->fd.start[(size_t)stream] = start_timestamp;
  return 0;
}

int adsb_stream_last_decoded(adsb_ctx* c, const adsb_decoded** rows, int32_t* n) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (!c->fd.open) return fail(c, -EINVAL, "adsb_stream_last_decoded: no streams (adsb_streams_open first)");
  if (rows) *rows = c->fd.n_rows > 0 ? (const adsb_decoded*)c->fd.h_rows.p : nullptr;
  if (n) *n = c->fd.n_rows;
  return 0;
}

int adsb_stream_decoder_reserve(adsb_ctx* c, int64_t slots) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  FleetDec& F = c->fd;
  if (!F.open) return fail(c, -EINVAL, "adsb_stream_decoder_reserve: no streams (adsb_streams_open first)");
  if (F.live_slots != 0) return fail(c, -EINVAL, "adsb_stream_decoder_reserve: the store holds live planes");
  if (slots < 0 || slots > kFleetMaxCap) return fail(c, -EINVAL, "adsb_stream_decoder_reserve: 0 .. 2^27 slots");
  long long cap = kFleetMinCap;
  while (cap < slots) cap *= 2;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  DevBuf fresh;
  int r;
  if ((r = fleet_new_store(c, fresh, cap)) || (r = fleet_take_store(c, fresh, cap))) return r;
  F.used = 0;
  return 0;
}

int adsb_stream_decoder_stats(adsb_ctx* c, int64_t* planes, int64_t* capacity, int64_t* grows) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (!c->fd.open) return fail(c, -EINVAL, "adsb_stream_decoder_stats: no streams (adsb_streams_open first)");
  if (planes) *planes = c->fd.live_planes;
  if (capacity) *capacity = c->fd.cap;
  if (grows) *grows = c->fd.grows;
  return 0;
}

int adsb_process_stream_batch_device(adsb_ctx* c, int format, const adsb_stream_item* items, int32_t n_items, adsb_burst* out,
                                     int32_t cap, int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  int rc = check_stream_batch(c, format, items, n_items, true, out, cap, item_first, n_out);
  if (rc) return rc;
  return run_stream_batch(c, format, items, n_items, true, out, cap, item_first, n_out, n_fallback);
}

int adsb_process_stream_batch(adsb_ctx* c, int format, const adsb_stream_item* items, int32_t n_items, adsb_burst* out, int32_t cap,
                              int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  int rc = check_stream_batch(c, format, items, n_items, false, out, cap, item_first, n_out);
  if (rc) return rc;
  rc = run_stream_batch(c, format, items, n_items, false, out, cap, item_first, n_out, n_fallback);
  // as adsb_process_batch: no upload that reads the CALLER's page-locked buffers is still queued when the call returns
  if (rc != 0 && rc != -ENOSPC) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int adsb_process_batch(adsb_ctx* c, int format, const adsb_batch_item* items, int32_t n_items, adsb_burst* out, int32_t cap,
                       int32_t* item_first, int32_t* n_out, int32_t* n_fallback) {
  int rc = check_batch(c, format, items, n_items, out, cap, item_first, n_out);
  if (rc) return rc;
  std::vector<adsb_batch_item> dev((size_t)n_items);
  if (n_items > 0) {
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = batch_slots_ok(c, items, n_items))) return rc;       // (before any upload is queued)
    rc = upload_batch(c, format, items, n_items, &dev);
    if (rc == 0) rc = run_batch(c, format, dev.data(), n_items, out, cap, item_first, n_out, n_fallback);
    // an error exit (an allocation that failed, ...) may leave uploads queued that read the CALLER's page-locked buffers:
    // they have finished when this call returns (a successful call and -ENOSPC have synchronised already)
    if (rc != 0 && rc != -ENOSPC) (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  return run_batch(c, format, dev.data(), n_items, out, cap, item_first, n_out, n_fallback);
}

static int shard_post(adsb_ctx* c, Slot& s, const Summary& sum, int32_t* nres_io, bool drop_overlong = false);

// The context's next pipeline slot takes the pass; the slot's number is the caller's ticket.
static int claim_and_enqueue(adsb_ctx* c, const Plan& pl, bool is_shard, int32_t* ticket) {
  Slot& s = c->slot[c->next_slot];
  const int r = enqueue(c, s, pl, true);
  if (r) return r;
  s.is_shard = is_shard;
  *ticket = c->next_slot;
  c->next_slot = (c->next_slot + 1) % ADSB_MAX_IN_FLIGHT;
  return 0;
}

static int submit_canonical(adsb_ctx* c, int mode, const void* d_data, int64_t n, int64_t abs_offset, int32_t* ticket) {
  if (!c || n < 1 || !ticket) return -EINVAL;
  if (((uintptr_t)d_data & 15u) != 0) return fail(c, -EINVAL, "device pointer must be 16-byte aligned");
  if (c->slot[c->next_slot].busy) return fail(c, -EBUSY, "every pipeline slot is in flight (adsb_wait first)");
  Plan pl = plan_canonical(mode, d_data, n, abs_offset, c->sps);
  pl.long_aware = (c->flags & ADSB_FLAG_LONG_AWARE_GATE) != 0;
  pl.air = (c->flags & ADSB_FLAG_AIRCRAFT_TABLE) != 0;
  return claim_and_enqueue(c, pl, false, ticket);
}

// Host buffer -> the slot's own device input buffer on the upload stream; only this slot's k_detect waits for it.
// Page-locked sources are DMA'd where they lie; pageable ones go through a ring of four pinned chunks: the host copy of
// chunk k+1 (split over the context's copy threads) runs beside the DMA of chunk k.
static int upload_async(adsb_ctx* c, Slot& s, const void* host, size_t bytes) {
  int rc;
  if ((rc = apply_ext(c, c->h2d_stream))) return rc;     // (the kernels come behind the upload: they need no wait of their own)
  if ((rc = ensure(c, s.d_in, bytes + 64))) return rc;
  if (is_pinned_host(host)) {
    HIPCHK(c, hipMemcpyAsync(s.d_in.p, host, bytes, hipMemcpyHostToDevice, c->h2d_stream));
  } else if ((rc = staged_copy(c, s.d_in.p, host, bytes, c->h2d_stream))) {
    return rc;
  }
  HIPCHK(c, hipEventRecord(s.h2d_done, c->h2d_stream));
  s.h2d_pending = true;          // enqueue() makes the stream this pass's k_detect runs on wait for it
  return 0;
}

int adsb_submit_format_host(adsb_ctx* c, int format, const void* host, int64_t n, int64_t abs_offset, int32_t* ticket) {
  if (!c || format < 0 || format >= ADSB_FMT_COUNT || n < 1 || !host || !ticket) return -EINVAL;
  Slot& s = c->slot[c->next_slot];
  if (s.busy) return fail(c, -EBUSY, "every pipeline slot is in flight (adsb_wait first)");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = upload_async(c, s, host, (size_t)n * (size_t)mode_bytes(format));
  if (rc) return rc;
  return submit_canonical(c, format, s.d_in.p, n, abs_offset, ticket);
}

int adsb_last_confidence(adsb_ctx* c, const float** ratio, int32_t* n) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_CONFIDENCE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_CONFIDENCE");
  const Slot& s = c->slot[c->last_slot];
  if (ratio) *ratio = s.nres > 0 ? (const float*)s.h_ratio.p : nullptr;
  if (n) *n = s.nres;
  return 0;
}

int adsb_set_soft_fec(adsb_ctx* c, const adsb_soft_fec_rule* rule) {
  if (!c) return -EINVAL;
  if (!(c->flags & (ADSB_FLAG_FEC_SOFT | ADSB_FLAG_FEC_SOFT_BATCH))) return fail(c, -EINVAL, "context created without ADSB_FLAG_FEC_SOFT / _FEC_SOFT_BATCH");
  if (!rule) return fail(c, -EINVAL, "rule");
  if (rule->n_weak < 1 || rule->n_weak > 16) return fail(c, -EINVAL, "soft rule: 1 <= n_weak <= 16");
  if (rule->max_flips < 1 || rule->max_flips > 5) return fail(c, -EINVAL, "soft rule: 1 <= max_flips <= 5");
  if (!(rule->min_key >= 0.0f && rule->min_key <= 1.0f)) return fail(c, -EINVAL, "soft rule: 0 <= min_key <= 1");
  if (rule->flags != 0u) return fail(c, -EINVAL, "soft rule: flags must be 0");
  { int r = require_idle(c, kCallPending); if (r) return r; }
  c->soft_rule = *rule;
  return 0;
}

int adsb_last_soft(adsb_ctx* c, const adsb_soft_fix** rows, int32_t* n) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_FEC_SOFT)) return fail(c, -EINVAL, "context created without ADSB_FLAG_FEC_SOFT");
  const Slot& s = c->slot[c->last_slot];
  if (c->soft_dm) { if (rows) *rows = c->soft_dm; if (n) *n = c->soft_dm_n; return 0; }
  if (rows) *rows = s.nres > 0 ? (const adsb_soft_fix*)s.h_soft.p : nullptr;
  if (n) *n = s.nres;
  return 0;
}

int adsb_batch_last_soft(adsb_ctx* c, const adsb_soft_fix** rows, int32_t* n) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_FEC_SOFT_BATCH)) return fail(c, -EINVAL, "context created without ADSB_FLAG_FEC_SOFT_BATCH");
  if (rows) *rows = c->batch_soft.empty() ? nullptr : c->batch_soft.data();
  if (n) *n = (int32_t)c->batch_soft.size();
  return 0;
}

int adsb_set_decoder(adsb_ctx* c, int32_t msg_filter, double start_timestamp) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_DECODE");
  if (msg_filter != ADSB_DEC_ALL_MESSAGES && msg_filter != ADSB_DEC_EXTENDED_SQUITTER_ONLY) return fail(c, -EINVAL, "msg_filter");
  { int r = require_idle(c, kCallPending); if (r) return r; }
  c->dec_all = msg_filter == ADSB_DEC_ALL_MESSAGES;
  c->dec_start = start_timestamp;
  return 0;
}

int adsb_last_decoded(adsb_ctx* c, const adsb_decoded** rows, int32_t* n) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_DECODE");
  const Slot& s = c->slot[c->last_slot];
  if (rows) *rows = s.nres > 0 ? (const adsb_decoded*)s.h_dec.p : nullptr;
  if (n) *n = s.nres;
  return 0;
}

int adsb_decode_pdus(adsb_ctx* c, const uint8_t* bits14, const double* timestamps, int32_t n, adsb_decoded* rows) {
  if (!c || n < 0 || (n > 0 && (!bits14 || !timestamps || !rows))) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_DECODE");
  int rc = require_idle(c, kCallPending);
  if (rc) return rc;
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  // staging in pinned, device-visible memory: rows (72 B) | timestamps (8 B) | bits (14 B) | ok (1 B) per PDU
  const size_t nt = (size_t)n, o_ts = nt * sizeof(adsb_decoded), o_bits = o_ts + nt * 8, o_ok = o_bits + nt * 14;
  if ((rc = ensure_pinned(c, c->h_pdu, o_ok + nt))) return rc;
  char* h = (char*)c->h_pdu.p;
  memcpy(h + o_ts, timestamps, nt * 8);
  memcpy(h + o_bits, bits14, nt * 14);
  if ((rc = apply_ext(c, c->stream))) return rc;
  const unsigned g = step_grid((long long)nt, kThreads);
  hipLaunchKernelGGL(k_dec_pdu_flags, dim3(g), dim3(kThreads), 0, c->stream, (const unsigned char*)(h + o_bits),
                     (unsigned char*)(h + o_ok), (int)n);
  if (c->flags & ADSB_FLAG_FEC_CONSERVATIVE)
    hipLaunchKernelGGL(k_fec_slices, dim3(g), dim3(kThreads), 0, c->stream, (unsigned char*)(h + o_bits),
                       (unsigned char*)(h + o_ok), (int)n);
  AirArgs aa{};
  aa.bits14 = (unsigned char*)(h + o_bits); aa.ok = (unsigned char*)(h + o_ok); aa.cap = (int)n;
  aa.pass = (c->air_next++) << 32;
  if ((rc = launch_air(c, c->stream, aa, (long long)n, (DecRow*)h, (const double*)(h + o_ts)))) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  hipError_t he = hipStreamSynchronize(c->stream);
  if (he == hipSuccess) he = hipGetLastError();
  if (he != hipSuccess) return fail(c, -EIO, "decode step", he);
  memcpy(rows, h, nt * sizeof(adsb_decoded));
  return 0;
}

// ---- snapshots of the plane tables (include/adsb_hip.h PLANE SNAPSHOTS; adsb_device.h: the k_planes_* kernels) --------------
// Both run on the context's stream behind the event of the last table / decode step and return when the rows are in the
// caller's memory; they write no state of the decoders.
// ages: the _seen variant (rows or last_seen may be missing, not both; the context has ADSB_FLAG_PLANE_AGES)
static int planes_args(adsb_ctx* c, const adsb_decoded* rows, int32_t cap, const int32_t* n_out, bool ages = false,
                       const int64_t* last_seen = nullptr) {
  if (!c) return -EINVAL;
  if (ages && !(c->flags & ADSB_FLAG_PLANE_AGES)) return fail(c, -EINVAL, "context created without ADSB_FLAG_PLANE_AGES");
  if (!n_out || cap < 0 || (cap > 0 && !rows && !last_seen)) return fail(c, -EINVAL, "plane snapshot: n_out, or rows for cap > 0, missing");
  return 0;
}

static int planes_dense(adsb_ctx* c, adsb_decoded* rows, int64_t* last_seen, bool ages, int32_t cap, int32_t* n_out) {
  int rc = planes_args(c, rows, cap, n_out, ages, last_seen);
  if (rc) return rc;
  if (!(c->flags & ADSB_FLAG_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_DECODE");
  if ((rc = require_idle(c, kCallPending))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = c->stream;
  PlanesDense a{};
  a.table = c->d_air; a.planes = c->d_planes; a.epoch = c->dec_epoch; a.lo = 0u; a.hi = 1u << 24;
  const unsigned n_chunks = (a.hi - a.lo) / kPlanesChunk;
  if ((rc = ensure(c, c->d_snap_cnt, ((size_t)n_chunks + 1) * sizeof(unsigned)))) return rc;
  unsigned* const cnt = (unsigned*)c->d_snap_cnt.p;
  const unsigned g = step_grid(n_chunks, kWaves);
  HIPCHK(c, hipStreamWaitEvent(st, c->air_ev, 0));
  hipLaunchKernelGGL(k_planes_tally, dim3(g), dim3(kThreads), 0, st, a, cnt);
  hipLaunchKernelGGL(k_dec_sort_scan, dim3(1), dim3(kThreads), 0, st, cnt, (int)n_chunks + 1);
  HIPCHK(c, hipGetLastError());
  unsigned total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, cnt + n_chunks, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  *n_out = (int32_t)total;
  if ((long long)total > (long long)cap) return fail(c, -ENOSPC, "adsb_planes: cap is smaller than the number of planes (*n_out)");
  if (total == 0) return 0;
  if (rows && (rc = ensure(c, c->d_snap_rows, (size_t)total * sizeof(DecRow)))) return rc;
  if (last_seen && (rc = ensure(c, c->d_snap_seen, (size_t)total * sizeof(long long)))) return rc;
  if (!ages)
    hipLaunchKernelGGL(k_planes_emit, dim3(g), dim3(kThreads), 0, st, a, (const unsigned*)cnt, (int)total, (DecRow*)c->d_snap_rows.p);
  else
    hipLaunchKernelGGL(k_ages_emit, dim3(g), dim3(kThreads), 0, st, a, (const unsigned*)cnt, (int)total,
                       rows ? (DecRow*)c->d_snap_rows.p : (DecRow*)nullptr, (const long long*)c->d_seen.p,
                       last_seen ? (long long*)c->d_snap_seen.p : (long long*)nullptr);
  HIPCHK(c, hipGetLastError());
  if (rows) HIPCHK(c, hipMemcpyAsync(rows, c->d_snap_rows.p, (size_t)total * sizeof(DecRow), hipMemcpyDeviceToHost, st));
  if (last_seen) HIPCHK(c, hipMemcpyAsync(last_seen, c->d_snap_seen.p, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

int adsb_planes(adsb_ctx* c, adsb_decoded* rows, int32_t cap, int32_t* n_out) { return planes_dense(c, rows, nullptr, false, cap, n_out); }
int adsb_planes_seen(adsb_ctx* c, adsb_decoded* rows, int64_t* last_seen, int32_t cap, int32_t* n_out) {
  return planes_dense(c, rows, last_seen, true, cap, n_out);
}

// del plane_dict[key] for every plane with last_seen < cutoff (adsb_device.h: plane ages), behind the last table / decode step
int adsb_planes_expire(adsb_ctx* c, int64_t cutoff, int64_t* n_removed) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_DECODE");
  if (!(c->flags & ADSB_FLAG_PLANE_AGES)) return fail(c, -EINVAL, "context created without ADSB_FLAG_PLANE_AGES");
  int rc = require_idle(c, kCallPending);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = c->stream;
  PlanesExpire a{};
  a.table = c->d_air; a.planes = c->d_planes; a.seen = c->d_seen; a.epoch = c->dec_epoch; a.lo = 0u; a.hi = 1u << 24;
  a.cutoff = (long long)cutoff;
  const unsigned n_chunks = (a.hi - a.lo) / kPlanesChunk;
  if ((rc = ensure(c, c->d_snap_cnt, ((size_t)n_chunks + 1) * sizeof(unsigned)))) return rc;
  unsigned long long* const d_n = (unsigned long long*)c->d_snap_cnt.p;      // (the snapshot's counts: no snapshot is at work)
  HIPCHK(c, hipStreamWaitEvent(st, c->air_ev, 0));
  HIPCHK(c, hipMemsetAsync(d_n, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_ages_expire, dim3(step_grid(n_chunks, kWaves)), dim3(kThreads), 0, st, a, d_n);
  HIPCHK(c, hipGetLastError());
  unsigned long long n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, d_n, sizeof(n), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (n_removed) *n_removed = (int64_t)n;
  return 0;
}

// The fleet calls' stream selection: the decoders are open; streams null selects all of them (*n_sel = their number), else
// *n_sel >= 0 indices, in range and strictly ascending.  api: the call's name in its refusals; cutoffs: null, or
// adsb_stream_planes_expire's (that call's n_sel refusal covers a missing *cutoffs too)
static int fleet_selection(adsb_ctx* c, const char* api, const int32_t* streams, int32_t* n_sel, const int64_t* const* cutoffs = nullptr) {
  const auto refuse = [&](const char* what) { snprintf(c->err, sizeof(c->err), "%s: %s", api, what); return -EINVAL; };
  if (!c->fd.open) return refuse("no streams (adsb_streams_open first)");
  const size_t ns = c->fd.gen.size();
  if (!streams) *n_sel = (int32_t)ns;
  if (*n_sel < 0 || (cutoffs && *n_sel > 0 && !*cutoffs)) return refuse(cutoffs ? "n_sel < 0, or cutoffs missing" : "n_sel < 0");
  for (int32_t i = 0; streams && i < *n_sel; ++i)
    if (streams[i] < 0 || (size_t)streams[i] >= ns || (i > 0 && streams[i] <= streams[i - 1]))
      return refuse("stream indices have to be in range and strictly ascending");
  return 0;
}

// The staging block of a fleet readout, in F.d_snap behind what is queued: generations | selection bitmap | with_list: selection
// list, first[] | count, error -- and room in F.d_keys / F.d_sorted for every live plane's key
struct FleetStage {
  PlanesFleet a{};
  int *sel = nullptr, *first = nullptr, *cnt = nullptr;     // on the device: the list and first[] (with_list), (count, error)
};
static int fleet_stage(adsb_ctx* c, const int32_t* streams, int32_t n_sel, bool with_list, FleetStage* sg) {
  FleetDec& F = c->fd;
  const size_t ns = F.gen.size(), nsel = with_list ? (size_t)n_sel : 0;
  const size_t o_bits = ns, o_sel = o_bits + (ns + 31) / 32, o_first = o_sel + nsel, o_cnt = o_first + (with_list ? nsel + 1 : 0), words = o_cnt + 2;
  std::vector<unsigned> h(words, 0u);
  for (size_t s = 0; s < ns; ++s) h[s] = F.gen[s];
  for (int32_t i = 0; streams && i < n_sel; ++i) {
    h[o_bits + (size_t)streams[i] / 32] |= 1u << ((unsigned)streams[i] & 31u);
    if (with_list) h[o_sel + (size_t)i] = (unsigned)streams[i];
  }
  const long long key_cap = F.live_planes;                     // every live plane is counted there (fleet_step)
  int rc;
  if ((rc = ensure(c, F.d_snap, words * sizeof(unsigned))) || (rc = ensure(c, F.d_keys, (size_t)key_cap * 8)) ||
      (rc = ensure(c, F.d_sorted, (size_t)key_cap * 8)))
    return rc;
  unsigned* const d = (unsigned*)F.d_snap.p;
  HIPCHK(c, hipMemcpyAsync(d, h.data(), words * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  sg->a.s = fleet_view(F.d_store.p, F.cap); sg->a.gen = d; sg->a.sel_bits = streams ? d + o_bits : nullptr; sg->a.n_streams = (int)ns;
  sg->sel = (int*)(d + o_sel); sg->first = (int*)(d + o_first); sg->cnt = (int*)(d + o_cnt);
  return 0;
}

// The selected planes' keys into F.d_keys (merge_seen null: k_planes_store_keys; else k_merge_keys, address-major, the planes
// seen before cutoff left out), their count read back into *n and checked against the streams' books, and for 1 .. limit keys
// the sort into F.d_sorted.  tmp_chunk: 0, or the keys per count of a later step that shares F.d_tmp with the sort.
static int fleet_sorted_keys(adsb_ctx* c, const FleetStage& sg, const long long* merge_seen, long long cutoff, int limit, int tmp_chunk, int* n_keys) {
  FleetDec& F = c->fd;
  const hipStream_t st = c->stream;
  const long long key_cap = F.live_planes;
  if (merge_seen)
    hipLaunchKernelGGL(k_merge_keys, dim3(step_grid(F.cap, kThreads)), dim3(kThreads), 0, st, sg.a, merge_seen, cutoff,
                       (unsigned long long*)F.d_keys.p, (int)key_cap, sg.cnt);
  else
    hipLaunchKernelGGL(k_planes_store_keys, dim3(step_grid(F.cap, kThreads)), dim3(kThreads), 0, st, sg.a, (unsigned long long*)F.d_keys.p,
                       (int)key_cap, sg.cnt);
  HIPCHK(c, hipGetLastError());
  int n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, sg.cnt, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if ((long long)n > key_cap) return fail(c, -EIO, "stream decoders: the store holds more planes than the streams count");
  *n_keys = n;
  if (n == 0 || n > limit) return 0;
  const size_t nblk = ((size_t)n + kSortTile - 1) / kSortTile, n_counts = tmp_chunk ? ((size_t)n + tmp_chunk - 1) / tmp_chunk + 1 : 0;
  int rc;
  if ((rc = ensure(c, F.d_tmp, std::max(nblk * 16, n_counts) * sizeof(unsigned)))) return rc;
  launch_key_sort(st, (unsigned long long*)F.d_keys.p, (unsigned long long*)F.d_sorted.p, n, 0, kFleetAddrBits + kFleetStreamBits, (unsigned*)F.d_tmp.p);
  return 0;
}

static int planes_fleet(adsb_ctx* c, const int32_t* streams, int32_t n_sel, adsb_decoded* rows, int64_t* last_seen, bool ages,
                        int32_t cap, int32_t* first, int32_t* n_out) {
  int rc = planes_args(c, rows, cap, n_out, ages, last_seen);
  if (rc) return rc;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if ((rc = fleet_selection(c, "adsb_stream_planes", streams, &n_sel)) || (rc = require_idle(c, kCallPending))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  FleetDec& F = c->fd;
  const hipStream_t st = c->stream;
  const size_t nsel = (size_t)n_sel;
  FleetStage sg;
  int n = 0;
  if ((rc = fleet_stage(c, streams, n_sel, true, &sg)) || (rc = fleet_sorted_keys(c, sg, nullptr, 0, cap, 0, &n))) return rc;
  *n_out = n;
  if (n > cap) return fail(c, -ENOSPC, "adsb_stream_planes: cap is smaller than the number of planes (*n_out)");
  if (n == 0) {
    if (first) memset(first, 0, (nsel + 1) * sizeof(int32_t));
    return 0;
  }
  if ((rows && (rc = ensure(c, F.d_rows, (size_t)n * sizeof(DecRow)))) || (last_seen && (rc = ensure(c, F.d_ages, (size_t)n * sizeof(long long)))))
    return rc;
  const int* const sel = streams ? sg.sel : nullptr;
  int* const d_first = first ? sg.first : nullptr;
  const unsigned eg = step_grid(std::max((long long)n, (long long)nsel + 1), kThreads);
  if (!ages)
    hipLaunchKernelGGL(k_planes_store_emit, dim3(eg), dim3(kThreads), 0, st, sg.a, (const unsigned long long*)F.d_sorted.p, n, sel, (int)n_sel,
                       (DecRow*)F.d_rows.p, d_first, sg.cnt + 1);
  else
    hipLaunchKernelGGL(k_ages_store_emit, dim3(eg), dim3(kThreads), 0, st, sg.a, (const unsigned long long*)F.d_sorted.p, n, sel, (int)n_sel,
                       rows ? (DecRow*)F.d_rows.p : (DecRow*)nullptr, d_first, sg.cnt + 1,
                       (const long long*)fleet_seen(c, F.d_store.p, F.cap), last_seen ? (long long*)F.d_ages.p : (long long*)nullptr);
  HIPCHK(c, hipGetLastError());
  int got[2] = {0, 0};
  if (rows) HIPCHK(c, hipMemcpyAsync(rows, F.d_rows.p, (size_t)n * sizeof(DecRow), hipMemcpyDeviceToHost, st));
  if (last_seen) HIPCHK(c, hipMemcpyAsync(last_seen, F.d_ages.p, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, st));
  if (first) HIPCHK(c, hipMemcpyAsync(first, sg.first, (nsel + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(got, sg.cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (got[1]) return fail(c, -EIO, "stream decoders: the snapshot found a plane without a slot");
  return 0;
}

int adsb_stream_planes(adsb_ctx* c, const int32_t* streams, int32_t n_sel, adsb_decoded* rows, int32_t cap, int32_t* first,
                       int32_t* n_out) {
  return planes_fleet(c, streams, n_sel, rows, nullptr, false, cap, first, n_out);
}
int adsb_stream_planes_seen(adsb_ctx* c, const int32_t* streams, int32_t n_sel, adsb_decoded* rows, int64_t* last_seen, int32_t cap,
                            int32_t* first, int32_t* n_out) {
  return planes_fleet(c, streams, n_sel, rows, last_seen, true, cap, first, n_out);
}

// The fleet's expiry: a rehash with a predicate into a store of the same size (adsb_device.h: plane ages)
int adsb_stream_planes_expire(adsb_ctx* c, const int32_t* streams, int32_t n_sel, const int64_t* cutoffs, int64_t* n_removed) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (!(c->flags & ADSB_FLAG_PLANE_AGES)) return fail(c, -EINVAL, "context created without ADSB_FLAG_PLANE_AGES");
  int rc;
  if ((rc = fleet_selection(c, "adsb_stream_planes_expire", streams, &n_sel, &cutoffs)) || (rc = require_idle(c, kCallPending))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  FleetDec& F = c->fd;
  std::vector<long long> cut(F.gen.size(), LLONG_MIN);                       // (nothing is below it: an unselected stream loses nothing)
  for (int32_t i = 0; i < n_sel; ++i) cut[streams ? (size_t)streams[i] : (size_t)i] = (long long)cutoffs[i];
  long long total = 0;
  if ((rc = fleet_rehash(c, F.cap, false, cut.data(), &total))) return rc;
  if (n_removed) *n_removed = (int64_t)total;
  return 0;
}

// The fleet's merged picture (adsb_device.h: k_merge_*): planes_fleet's shape with the address-major key, a head count and its
// scan between the sort and the emit step
static_assert(sizeof(adsb_merged) == 32 && sizeof(adsb_merged) == sizeof(MergedInfo), "adsb_merged is 32 bytes");
int adsb_stream_planes_merged(adsb_ctx* c, const int32_t* streams, int32_t n_sel, int64_t cutoff, adsb_decoded* rows, adsb_merged* info,
                              int32_t cap, int32_t* n_out) {
  if (!c) return -EINVAL;
  if (!(c->flags & ADSB_FLAG_STREAM_DECODE)) return fail(c, -EINVAL, "context created without ADSB_FLAG_STREAM_DECODE");
  if (!(c->flags & ADSB_FLAG_PLANE_AGES)) return fail(c, -EINVAL, "context created without ADSB_FLAG_PLANE_AGES");
  if (!n_out || cap < 0 || (cap > 0 && !rows && !info)) return fail(c, -EINVAL, "adsb_stream_planes_merged: n_out, or rows / info for cap > 0, missing");
  int rc;
  if ((rc = fleet_selection(c, "adsb_stream_planes_merged", streams, &n_sel)) || (rc = require_idle(c, kCallPending))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  FleetDec& F = c->fd;
  const hipStream_t st = c->stream;
  const long long* const seen = fleet_seen(c, F.d_store.p, F.cap);
  FleetStage sg;
  int n = 0;
  if ((rc = fleet_stage(c, streams, n_sel, false, &sg)) || (rc = fleet_sorted_keys(c, sg, seen, (long long)cutoff, INT_MAX, kMergeChunk, &n)))
    return rc;
  if (n == 0) {
    *n_out = 0;
    return 0;
  }
  const int n_chunks = (n + kMergeChunk - 1) / kMergeChunk;
  const unsigned eg = step_grid(n, kThreads);
  hipLaunchKernelGGL(k_merge_heads, dim3(eg), dim3(kThreads), 0, st, (const unsigned long long*)F.d_sorted.p, n, (unsigned*)F.d_tmp.p);
  hipLaunchKernelGGL(k_dec_sort_scan, dim3(1), dim3(kThreads), 0, st, (unsigned*)F.d_tmp.p, n_chunks + 1);
  HIPCHK(c, hipGetLastError());
  unsigned total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, (unsigned*)F.d_tmp.p + n_chunks, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (total == 0 || total > (unsigned)n) return fail(c, -EIO, "stream decoders: the merged picture's head count is out of range");
  *n_out = (int32_t)total;
  if (total > (unsigned)cap) return fail(c, -ENOSPC, "adsb_stream_planes_merged: cap is smaller than the number of aircraft (*n_out)");
  if ((rows && (rc = ensure(c, F.d_rows, (size_t)total * sizeof(DecRow)))) || (info && (rc = ensure(c, F.d_merged, (size_t)total * sizeof(MergedInfo)))))
    return rc;
  hipLaunchKernelGGL(k_merge_emit, dim3(eg), dim3(kThreads), 0, st, sg.a, (const unsigned long long*)F.d_sorted.p, n,
                     (const unsigned*)F.d_tmp.p, seen, rows ? (DecRow*)F.d_rows.p : (DecRow*)nullptr,
                     info ? (MergedInfo*)F.d_merged.p : (MergedInfo*)nullptr, sg.cnt + 1);
  HIPCHK(c, hipGetLastError());
  int got[2] = {0, 0};
  if (rows) HIPCHK(c, hipMemcpyAsync(rows, F.d_rows.p, (size_t)total * sizeof(DecRow), hipMemcpyDeviceToHost, st));
  if (info) HIPCHK(c, hipMemcpyAsync(info, F.d_merged.p, (size_t)total * sizeof(MergedInfo), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(got, sg.cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (got[1]) return fail(c, -EIO, "stream decoders: the merged picture found a plane without a slot");
  return 0;
}

int adsb_submit_format_device(adsb_ctx* c, int format, const void* d_data, int64_t n, int64_t abs_offset, int32_t* ticket) {
  if (!c || format < 0 || format >= ADSB_FMT_COUNT) return -EINVAL;
  return submit_canonical(c, format, d_data, n, abs_offset, ticket);
}

int adsb_wait(adsb_ctx* c, int32_t ticket, adsb_burst* out, int32_t cap, int32_t* n_out) {
  if (!c || ticket < 0 || ticket >= ADSB_MAX_IN_FLIGHT) return -EINVAL;
  Slot& s = c->slot[ticket];
  if (!s.busy) return fail(c, -EINVAL, "no call pending on this ticket");
  Summary sum;
  int32_t nres = 0;
  int r = finish(c, s, &sum, &nres);
  if (r) return r;
  c->last_slot = ticket;
  if (s.is_shard && (r = shard_post(c, s, sum, &nres))) return r;
  return deliver(c, nres, out, cap, n_out);
}

int adsb_last_result(adsb_ctx* c, const adsb_burst** bursts, int32_t* n) {
  if (!c) return -EINVAL;
  if (bursts) *bursts = (const adsb_burst*)c->slot[c->last_slot].h_out.p;
  if (n) *n = c->slot[c->last_slot].nres;
  return 0;
}

int adsb_framer_work(adsb_ctx* c, const float* in0, int64_t n_in0, int64_t N, int64_t nitems_written,
                     adsb_burst* tags, int32_t cap, int32_t* n_out) {
  return adsb_framer_work_passthrough(c, in0, n_in0, N, nitems_written, nullptr, tags, cap, n_out);
}

int adsb_framer_work_passthrough(adsb_ctx* c, const float* in0, int64_t n_in0, int64_t N, int64_t nitems_written, float* out0,
                                 adsb_burst* tags, int32_t cap, int32_t* n_out) {
  if (!c || !in0 || N < 1) return -EINVAL;
  if (c->flags & ADSB_FLAG_DECODE) return fail(c, -EINVAL, "adsb_framer_work is not for ADSB_FLAG_DECODE contexts");
  const long long H = 8ll * c->sps;
  if (n_in0 != N + H - 1) return fail(c, -EINVAL, "framer input must hold N + 8*sps - 1 items");
  HIPCHK(c, hipSetDevice(c->device));
  void* d = nullptr;
  int rc = upload(c, in0, (size_t)n_in0 * 4, &d);
  if (rc) return rc;
  Plan pl = plan_framer_work(d, n_in0, N, nitems_written, c->sps, c->st);
  if (c->flags & ADSB_FLAG_FRAMER_SLICES) pl.dem_hi = n_in0;   // bursts that end inside this call's input get their bits
  Summary s;
  int32_t nres = 0;
  if ((rc = require_idle(c, kCallPending))) return rc;
  {
    // the device pass is queued, THEN the block's pass-through copy (framer.py:181: out0[:] = in0[history:]) runs on the
    // host -- beside the upload's DMA and the kernels instead of behind them -- then the pass is waited for
    Slot& sl0 = c->slot[0];
    c->last_slot = 0;
    if ((rc = enqueue(c, sl0, pl, false))) return rc;
    if (out0) {
      const size_t pb = (size_t)N * sizeof(float);
      if (pb >= ((size_t)1 << 20) && ensure_pool(c) == 0) c->pool->copy((char*)out0, (const char*)(in0 + (H - 1)), pb);
      else memcpy(out0, in0 + (H - 1), pb);
    }
    rc = finish(c, sl0, &s, &nres);
  }
  if (rc) return rc;
  // cross-call state, exactly as framer.py:87,121-123,165,177-179 (in0 index == local index here)
  framer_state_update(c->st, in0[N - 1], N, c->sps, s.flags, s.lastp, kNoIndex, nres,
                      nres > 0 ? s.last_kept_p : 0);
  return deliver(c, nres, tags, cap, n_out);
}

int adsb_demod_work(adsb_ctx* c, const float* in0, int64_t n, int64_t nitems_read, const int64_t* tag_offsets,
                    int32_t ntags, uint8_t* bits112, uint8_t* ok, float* ratio) {
  if (!c || n < 0 || ntags < 0 || (n > 0 && !in0) || (ntags > 0 && (!tag_offsets || !bits112 || !ok))) return -EINVAL;
  if (c->flags & ADSB_FLAG_DECODE) return fail(c, -EINVAL, "adsb_demod_work is not for ADSB_FLAG_DECODE contexts (adsb_decode_pdus)");
  if (ntags == 0) return 0;
  int rc;
  // (the table steps of passes in flight may still be settled: finish)
  if ((c->flags & ADSB_FLAG_AIRCRAFT_TABLE) && (rc = require_idle(c, kCallPending))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // (independent of submitted calls still in flight: own buffers, ordered behind them on the compute stream)
  // Tag positions, packed bits, ok flags and ratios live in the context's pinned, device-visible scratch (layout: tag
  // positions | packed bits | ok | ratios): the kernel reads and writes them in place, so the call is one sample upload,
  // one kernel and ONE synchronisation.  Every buffer is acquired BEFORE anything is queued: no error path leaves work
  // in flight.
  const size_t nt = (size_t)ntags;
  const size_t o_bits = nt * 8, o_ok = o_bits + nt * 14, o_ratio = (o_ok + nt + 15) & ~(size_t)15;
  const size_t o_soft = (o_ratio + (ratio ? nt * 112 * sizeof(float) : 0) + 15) & ~(size_t)15;      // ADSB_FLAG_FEC_SOFT: the tags' rows
  const size_t total = (c->flags & ADSB_FLAG_FEC_SOFT) ? o_soft + nt * sizeof(adsb_soft_fix) : o_ratio + (ratio ? nt * 112 * sizeof(float) : 0);
  if ((rc = ensure_pinned(c, c->h_dm, total))) return rc;
  c->soft_dm = nullptr;
  char* h = (char*)c->h_dm.p;
  long long* loc = (long long*)h;
  // local positions of the tags inside in0 (demod.py:79: offset - nitems_written); a tag outside the chunk -- the
  // reference's get_tags_in_range never returns one (demod.py:67) -- is dropped by the kernel (ok = 0)
  for (int t = 0; t < ntags; ++t) loc[t] = tag_offsets[t] - nitems_read;
  void* d = nullptr;
  if ((rc = upload(c, in0, (size_t)n * 4, &d))) return rc;
  hipLaunchKernelGGL((k_slice<1>), dim3(step_grid(ntags, kWaves)), dim3(kThreads), 0, c->stream, (const void*)d, (long long)n,
                     (const long long*)loc, (int)ntags, c->sps, (unsigned char*)(h + o_bits),
                     (unsigned char*)(h + o_ok), ratio ? (float*)(h + o_ratio) : (float*)nullptr);
  if (c->flags & ADSB_FLAG_FEC_CONSERVATIVE)
    hipLaunchKernelGGL(k_fec_slices, dim3(step_grid(ntags, kThreads)), dim3(kThreads), 0, c->stream, (unsigned char*)(h + o_bits),
                       (unsigned char*)(h + o_ok), (int)ntags);
  if (c->flags & ADSB_FLAG_FEC_SOFT) {
    const int e = adsb_softfec_host::launch_slices(c->stream, step_grid(ntags, kWaves), d, (long long)n, (const long long*)loc, c->sps, &c->soft_rule,
                                                   (unsigned char*)(h + o_bits), (unsigned char*)(h + o_ok), (int)ntags, h + o_soft);
    if (e) { (void)hipStreamSynchronize(c->stream); return fail(c, -EIO, "soft repair launch", (hipError_t)e); }
  }
  if (c->flags & ADSB_FLAG_AIRCRAFT_TABLE) {
    // the slices with ok != 0 are this call's published PDUs, in tag order
    AirArgs aa{};
    aa.bits14 = (unsigned char*)(h + o_bits); aa.ok = (unsigned char*)(h + o_ok); aa.cap = (int)ntags;
    aa.pass = (c->air_next++) << 32;
    if ((rc = launch_air(c, c->stream, aa, (long long)ntags))) { (void)hipStreamSynchronize(c->stream); return rc; }
  }
  hipError_t he = hipStreamSynchronize(c->stream);            // always: nothing stays queued behind an error return
  if (he == hipSuccess) he = hipGetLastError();
  if (he != hipSuccess) return fail(c, -EIO, "k_slice", he);
  const unsigned char* packed = (const unsigned char*)(h + o_bits);
  for (size_t t = 0; t < nt; ++t)
    for (int k = 0; k < 112; ++k) bits112[t * 112 + k] = (packed[t * 14 + (k >> 3)] >> (7 - (k & 7))) & 1u;
  memcpy(ok, h + o_ok, nt);
  if (c->flags & ADSB_FLAG_FEC_SOFT) { c->soft_dm = (const adsb_soft_fix*)(h + o_soft); c->soft_dm_n = (int32_t)ntags; }
  if (ratio) {
    memcpy(ratio, h + o_ratio, nt * 112 * sizeof(float));
    for (size_t t = 0; t < nt; ++t)                            // the kernel leaves the rows of dropped tags untouched
      if (!ok[t]) memset(ratio + t * 112, 0, 112 * sizeof(float));
  }
  return 0;
}

// Halo checks of a finished shard call (the records are in the slot's pinned buffer).  drop_overlong
// (ADSB_SHARD_DROP_OVERLONG): a centre whose pulse or burst runs past the buffer's forward halo is left out of the
// result instead of failing the call -- the reference degrades the same way (a pulse still high at the end of a
// call is never evaluated, framer.py:102-108; a burst past the end of the chunk is dropped, demod.py:130-133).
static int shard_post(adsb_ctx* c, Slot& s, const Summary& sum, int32_t* nres_io, bool drop_overlong) {
  if ((sum.flags & 4u) && !drop_overlong) return fail(c, -EOVERFLOW, "pulse runs past the shard's forward halo");
  Rec* r = (Rec*)s.h_out.p;
  const int32_t nres = *nres_io;
  const long long origin = s.plan.origin, n = s.plan.n, stream_len = s.plan.origin + s.plan.dem_hi;
  int32_t w = 0;
  for (int i = 0; i < nres; ++i) {
    const unsigned fl = (unsigned)(r[i].w[3] >> 48);
    const long long off = (long long)r[i].w[0];
    const long long eob = off + 119ll * c->sps + c->sps / 2;
    if (!(fl & kDemod) && eob < stream_len) return fail(c, -EOVERFLOW, "internal: demod flag");
    if ((fl & kDemod) && eob >= origin + n) {
      if (drop_overlong) continue;
      return fail(c, -EOVERFLOW, "burst runs past the shard's forward halo");
    }
    if (off - 100 < origin && origin > 0) return fail(c, -EOVERFLOW, "noise window runs past the shard's back halo");
    if (w != i) {
      r[w] = r[i];
      // row t of adsb_last_confidence belongs to record t of the delivered list: rows move with their records
      if ((c->flags & ADSB_FLAG_CONFIDENCE) && s.h_ratio.p) memcpy((float*)s.h_ratio.p + (size_t)w * 112, (float*)s.h_ratio.p + (size_t)i * 112, 112 * sizeof(float));
      if ((c->flags & ADSB_FLAG_FEC_SOFT) && s.h_soft.p) ((adsb_soft_fix*)s.h_soft.p)[w] = ((adsb_soft_fix*)s.h_soft.p)[i];
    }
    ++w;
  }
  s.nres = w;
  *nres_io = w;
  return 0;
}

// What every sharded entry point refuses, each stated once: a context with an aircraft table, a device pointer (where the
// call has one yet) off a 16-byte boundary, and -- the two drivers, by their own name -- a confidence context.  The text
// goes to `err_to` where that is another context.
static int shard_refused(adsb_ctx* c, const void* d_data, adsb_ctx* err_to = nullptr) {
  if (c->flags & ADSB_FLAG_AIRCRAFT_TABLE) return fail(err_to ? err_to : c, -EINVAL, "sharded calls are not for ADSB_FLAG_AIRCRAFT_TABLE contexts");
  if (((uintptr_t)d_data & 15u) != 0) return fail(err_to ? err_to : c, -EINVAL, "device pointer must be 16-byte aligned");
  return 0;
}
static int confidence_refused(adsb_ctx* c, const char* entry, adsb_ctx* err_to) {
  if (!(c->flags & (ADSB_FLAG_CONFIDENCE | ADSB_FLAG_FEC_SOFT))) return 0;
  snprintf(err_to->err, sizeof(err_to->err), "%s: not for %s contexts", entry, (c->flags & ADSB_FLAG_CONFIDENCE) ? "ADSB_FLAG_CONFIDENCE" : "ADSB_FLAG_FEC_SOFT");
  return -EINVAL;
}

static int shard_plan_checked(adsb_ctx* c, int fmt, const void* d_data, int64_t n, int64_t origin, int64_t own_lo,
                              int64_t own_hi, int64_t stream_len, int32_t head_cands, Plan* pl) {
  if (!c || n < 0 || fmt < 0 || fmt >= ADSB_FMT_COUNT || head_cands < 0) return -EINVAL;
  if (int r = shard_refused(c, d_data)) return r;
  *pl = plan_shard(fmt, d_data, n, origin, own_lo, own_hi, stream_len, c->sps, head_cands);
  pl->long_aware = (c->flags & ADSB_FLAG_LONG_AWARE_GATE) != 0;
  if (origin > 0 && pl->scan_lo < 1) return fail(c, -EINVAL, "shard needs at least one sample of back halo");
  return 0;
}

// a queued shard pass, finished: its slot is the last slot, and its records -- in the slot's pinned buffer -- have passed
// shard_post
static int collect_pass(adsb_ctx* c, int32_t ticket, adsb_burst** recs, int32_t* nres) {
  Slot& s = c->slot[ticket];
  Summary sum;
  *nres = 0;
  int r = finish(c, s, &sum, nres);
  if (r) return r;
  c->last_slot = ticket;
  if ((r = shard_post(c, s, sum, nres))) return r;
  *recs = (adsb_burst*)s.h_out.p;
  return 0;
}

// the tail of the blocking shard calls: the pass, its halo checks, its records
static int shard_run(adsb_ctx* c, const Plan& pl, bool drop_overlong, adsb_burst* out, int32_t cap, int32_t* n_out) {
  Summary s;
  int32_t nres = 0;
  int rc = run_pipeline(c, pl, &s, &nres);
  if (rc) return rc;
  if ((rc = shard_post(c, c->slot[c->last_slot], s, &nres, drop_overlong))) return rc;
  return deliver(c, nres, out, cap, n_out);
}

int adsb_shard_device(adsb_ctx* c, int fmt, const void* d_data, int64_t n, int64_t origin, int64_t own_lo,
                      int64_t own_hi, int64_t stream_len, int32_t head_cands, adsb_burst* out, int32_t cap,
                      int32_t* n_out) {
  Plan pl;
  int rc = shard_plan_checked(c, fmt, d_data, n, origin, own_lo, own_hi, stream_len, head_cands, &pl);
  if (rc) return rc;
  return shard_run(c, pl, false, out, cap, n_out);
}

int adsb_shard_host(adsb_ctx* c, int fmt, const void* host, int64_t n, int64_t origin, int64_t own_lo, int64_t own_hi,
                    int64_t stream_len, int32_t head_cands, uint32_t shard_flags, adsb_burst* out, int32_t cap,
                    int32_t* n_out) {
  if (!c || fmt < 0 || fmt >= ADSB_FMT_COUNT || n < 1 || !host) return -EINVAL;
  int rc = shard_refused(c, nullptr);          // (before the upload: no device pointer yet)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  void* d = nullptr;
  if ((rc = upload(c, host, (size_t)n * (size_t)mode_bytes(fmt), &d))) return rc;
  Plan pl;
  if ((rc = shard_plan_checked(c, fmt, d, n, origin, own_lo, own_hi, stream_len, head_cands, &pl))) return rc;
  return shard_run(c, pl, (shard_flags & ADSB_SHARD_DROP_OVERLONG) != 0, out, cap, n_out);
}

int adsb_submit_shard_device(adsb_ctx* c, int fmt, const void* d_data, int64_t n, int64_t origin, int64_t own_lo,
                             int64_t own_hi, int64_t stream_len, int32_t head_cands, int32_t* ticket) {
  if (!ticket) return -EINVAL;
  Plan pl;
  int rc = shard_plan_checked(c, fmt, d_data, n, origin, own_lo, own_hi, stream_len, head_cands, &pl);
  if (rc) return rc;
  if (c->slot[c->next_slot].busy) return fail(c, -EBUSY, "every pipeline slot is in flight (adsb_wait first)");
  return claim_and_enqueue(c, pl, true, ticket);
}

int32_t adsb_shard_bounds(int64_t stream_len, int32_t n_shards, int32_t g, int sps, int64_t align, int64_t* own_lo,
                          int64_t* own_hi, int64_t* lo, int64_t* hi) {
  // The tiling of gr_adsb_amd/frontend.py: shard_plan (one rule for every caller: bench.py's ranks, file replay, the C
  // driver below): equal owner ranges of a multiple of `align` samples; back halo = noise window + preamble span + 4
  // (framer.py:31,137-147), buffer start on a 16-byte boundary of every format; forward halo = longest pulse followed (256)
  // + preamble and 112 bits (121*sps: framer.py:165, demod.py:76).
  if (stream_len < 0 || n_shards < 1 || g < 0 || g >= n_shards || sps < 2 || align < 1 || !own_lo || !own_hi || !lo || !hi) return -EINVAL;
  long long per = (stream_len + n_shards - 1) / n_shards;
  per = (per + align - 1) / align * align;
  const long long olo = (long long)g * per < stream_len ? (long long)g * per : stream_len;
  const long long ohi = (long long)(g + 1) * per < stream_len ? (long long)(g + 1) * per : stream_len;
  long long l = olo - (kNoise + 8ll * sps + 4);
  if (l < 0) l = 0;
  l -= l % 4;
  long long h = ohi + 256 + 121ll * sps;
  if (h > stream_len) h = stream_len;
  *own_lo = olo; *own_hi = ohi; *lo = l; *hi = h;
  return 0;
}

int adsb_process_sharded_device(adsb_ctx* c, int fmt, const void* d_data, int64_t n, int64_t abs_offset, int32_t shards,
                                adsb_burst* out, int32_t cap, int32_t* n_out) {
  if (!c || fmt < 0 || fmt >= ADSB_FMT_COUNT || n < 0 || shards < 1 || cap < 0 || (cap > 0 && !out) || !n_out) return -EINVAL;
  int rc = shard_refused(c, d_data);
  if (rc || (rc = require_idle(c, kCallPending))) return rc;
  // the rows of adsb_last_confidence belong to the records of ONE pass in the order that pass delivered them; this driver
  // re-gates and concatenates the records of many passes on the host
  if ((rc = confidence_refused(c, "adsb_process_sharded_device", c))) return rc;
  *n_out = 0;
  if (n == 0) return 0;
  // adsb_wait_for_event: EVERY shard pass reads the caller's buffer and the passes run on different streams, so every
  // one of them (the re-runs of the fallback included) waits for the pending events -- enqueue() applies and clears what
  // is pending, the driver puts the same events back in front of each of its passes
  hipEvent_t ext_snap[adsb_ctx::kMaxExt];
  const int n_ext_snap = c->n_ext;
  for (int i = 0; i < n_ext_snap; ++i) ext_snap[i] = c->ext_ev[i];
  auto rearm = [&]() { for (int i = 0; i < n_ext_snap; ++i) c->ext_ev[i] = ext_snap[i]; c->n_ext = n_ext_snap; };
  const int bps = mode_bytes(fmt);
  struct Pend { int ticket; long long own_lo, own_hi, lo, hi; };
  Pend pend[ADSB_MAX_IN_FLIGHT];
  int n_pend = 0, head = 0;
  SeamConsumer seam{c->sps, out, cap, abs_offset};

  // collect the oldest pass: the seam consumer fixes up its head with the carried state and appends what it kept
  auto collect = [&]() -> int {
    const Pend p = pend[head];
    head = (head + 1) % ADSB_MAX_IN_FLIGHT; --n_pend;
    adsb_burst* recs = nullptr;
    int32_t nres = 0, kept = 0;
    int r = collect_pass(c, p.ticket, &recs, &nres);
    if (r) return r;
    // a head that ended inside a chain: this shard again on the slot that has just become free
    int rerun_rc = 0;
    auto rerun = [&](int head_cands, adsb_burst** rr, int32_t* nn) -> int {
      Plan pl;
      int e = shard_plan_checked(c, fmt, (const char*)d_data + (size_t)p.lo * bps, p.hi - p.lo, p.lo, p.own_lo, p.own_hi, n, head_cands, &pl);
      if (!e) { rearm(); e = enqueue(c, c->slot[p.ticket], pl, true); }
      if (!e) e = collect_pass(c, p.ticket, rr, nn);
      return rerun_rc = e;
    };
    if ((r = seam.take(recs, nres, rerun, &kept))) return rerun_rc ? r : fail(c, r, "adsb_shard_fixup");   // (a failed re-run keeps its pass's text)
    c->slot[p.ticket].nres = kept;
    return 0;
  };

  for (int32_t g = 0; g < shards && !rc; ++g) {
    int64_t own_lo, own_hi, lo, hi;
    if ((rc = adsb_shard_bounds(n, shards, g, c->sps, 4096, &own_lo, &own_hi, &lo, &hi))) break;
    if (own_hi <= own_lo) continue;
    if (n_pend == ADSB_MAX_IN_FLIGHT && (rc = collect())) break;
    Plan pl;
    if ((rc = shard_plan_checked(c, fmt, (const char*)d_data + (size_t)lo * bps, hi - lo, lo, own_lo, own_hi, n, kHeadFirst, &pl))) break;
    int32_t ticket = -1;
    rearm();
    if ((rc = claim_and_enqueue(c, pl, true, &ticket))) break;
    pend[(head + n_pend) % ADSB_MAX_IN_FLIGHT] = Pend{ticket, own_lo, own_hi, lo, hi};
    ++n_pend;
  }
  while (n_pend > 0) {
    const int r = collect();          // (after an error too: no pass stays in flight behind this call)
    if (r && !rc) rc = r;
  }
  c->n_ext = 0;                       // consumed by this call, whether a pass was queued or not
  c->stats.shard_fallbacks += seam.fallbacks;
  if (rc) return rc;
  return seam.finish(n_out) ? fail(c, -ENOSPC, "output array too small") : 0;
}

// ---- one process, N devices, one host ring (BASELINE config 4) --------------------------------------------
// The stream lies in HOST memory; context k (one per device, or several on one) takes `shards_per_ctx` consecutive
// overlapped time shards of it.  One feeder thread per context, inside the cpus local to its GPU: upload of shard i+1 on
// the context's upload stream beside the shard pass of i and the record download of i-1, ADSB_MAX_IN_FLIGHT deep -- the
// host-fed pipeline of adsb_submit_format_host with a shard plan.  The calling thread takes the finished shards in STREAM
// order as they arrive and re-gates each head with the end-of-burst state carried over the seam (adsb_seam.h: SeamConsumer); a head
// that ends inside an unbroken chain has its shard run again on its own context (largest head, then ungated + the plain
// greedy gate), after that context's feeder has finished.  No interpreter, no torch.distributed, no mailbox: the only
// thing that crosses a seam is one int64.
namespace {

struct MultiShard {
  long long own_lo = 0, own_hi = 0, lo = 0, hi = 0;
  std::vector<adsb_burst> recs;      // the shard's records as its pass delivered them (head + what a fresh-state gate kept)
  int rc = 0;
  bool done = false;
};

// queue one shard of a host-resident stream on the context's next slot: upload -> shard pass
int submit_shard_host(adsb_ctx* c, int fmt, const char* host, const MultiShard& sh, long long stream_len, int head, int32_t* ticket) {
  Slot& s = c->slot[c->next_slot];
  if (s.busy) return fail(c, -EBUSY, "every pipeline slot is in flight");
  HIPCHK(c, hipSetDevice(c->device));
  const int bps = mode_bytes(fmt);
  int rc = upload_async(c, s, host + (size_t)sh.lo * bps, (size_t)(sh.hi - sh.lo) * bps);
  if (rc) return rc;
  Plan pl;
  if ((rc = shard_plan_checked(c, fmt, s.d_in.p, sh.hi - sh.lo, sh.lo, sh.own_lo, sh.own_hi, stream_len, head, &pl))) return rc;
  return claim_and_enqueue(c, pl, true, ticket);
}

int collect_shard(adsb_ctx* c, int32_t ticket, std::vector<adsb_burst>* out) {
  adsb_burst* recs = nullptr;
  int32_t nres = 0;
  const int r = collect_pass(c, ticket, &recs, &nres);
  if (r) return r;
  try {
    out->assign(recs, recs + nres);
  } catch (...) {                                     // (no exception crosses the ABI or ends a feeder thread)
    return fail(c, -ENOMEM, "shard records");
  }
  return 0;
}

}  // namespace

int adsb_process_sharded_multi(adsb_ctx* const* ctxs, int32_t n_ctx, int fmt, const void* host, int64_t n, int64_t abs_offset,
                               int32_t shards_per_ctx, adsb_burst* out, int32_t cap, int32_t* n_out, adsb_multi_stats* stats) {
  if (!ctxs || n_ctx < 1 || n_ctx > ADSB_MULTI_MAX_CTX || fmt < 0 || fmt >= ADSB_FMT_COUNT || n < 0 || shards_per_ctx < 1 ||
      cap < 0 || (cap > 0 && !out) || !n_out || (n > 0 && !host)) return -EINVAL;
  adsb_ctx* c0 = ctxs[0];
  if (!c0) return -EINVAL;
  for (int k = 0; k < n_ctx; ++k) {
    adsb_ctx* c = ctxs[k];
    if (!c) return -EINVAL;
    for (int j = 0; j < k; ++j) if (ctxs[j] == c) return fail(c0, -EINVAL, "adsb_process_sharded_multi: a context listed twice");
    if (shard_refused(c, nullptr, c0)) return -EINVAL;
    // one stream, one set of rules: every context must have been created with the same rate, threshold, gate and scale
    if (c->sps != c0->sps || !(c->thr == c0->thr) || ((c->flags ^ c0->flags) & (ADSB_FLAG_LONG_AWARE_GATE | ADSB_FLAG_FEC_CONSERVATIVE)) ||
        !(c->scale[fmt] == c0->scale[fmt]))
      return fail(c0, -EINVAL, "adsb_process_sharded_multi: contexts differ in rate, threshold, gate, FEC or format scale");
    if (confidence_refused(c, "adsb_process_sharded_multi", c0)) return -EINVAL;
    if (!c->own_stream) return fail(c0, -EINVAL, "adsb_process_sharded_multi: not for contexts on a caller-owned stream");
    if (require_idle(c, "a submitted call is still pending on one of the contexts", c0)) return -EBUSY;
  }
  *n_out = 0;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (n == 0) return 0;
  const int sps = c0->sps;
  const int G = n_ctx * shards_per_ctx;
  const auto t_start = std::chrono::steady_clock::now();

  std::vector<MultiShard> sh;
  std::vector<double> feed_s;
  std::vector<std::thread> th;
  std::vector<char> joined;
  try {
    sh.resize((size_t)G); feed_s.assign((size_t)n_ctx, 0.0); th.reserve((size_t)n_ctx); joined.assign((size_t)n_ctx, 0);
  } catch (...) {
    return fail(c0, -ENOMEM, "adsb_process_sharded_multi: shard table");
  }
  for (int g = 0; g < G; ++g) {
    int64_t olo, ohi, lo, hi;
    const int rc = adsb_shard_bounds(n, G, g, sps, 4096, &olo, &ohi, &lo, &hi);
    if (rc) return rc;
    sh[(size_t)g].own_lo = olo; sh[(size_t)g].own_hi = ohi; sh[(size_t)g].lo = lo; sh[(size_t)g].hi = hi;
  }
  std::mutex m;
  std::condition_variable cv;

  // context k's feeder: its shards, ADSB_MAX_IN_FLIGHT deep.  An error ends this feeder only (its remaining shards are
  // marked done with the error) -- and nothing of its context stays in flight behind it.
  auto feeder = [&](int k) {
    adsb_ctx* c = ctxs[k];
    if (c->have_local_cpus && !(c->flags & ADSB_FLAG_NO_NUMA_BINDING)) {
      cpu_set_t mine, both;
      CPU_ZERO(&mine);
      if (sched_getaffinity(0, sizeof(mine), &mine) == 0) {
        CPU_AND(&both, &mine, &c->local_cpus);
        if (CPU_COUNT(&both) > 0) (void)pthread_setaffinity_np(pthread_self(), sizeof(both), &both);
      }
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int g0 = k * shards_per_ctx, g1 = g0 + shards_per_ctx;
    struct Fly { int g; int32_t ticket; };
    Fly fly[ADSB_MAX_IN_FLIGHT];
    int n_fly = 0, head = 0, rc = 0;
    auto mark = [&](int g, int r) {
      { std::lock_guard<std::mutex> lk(m); sh[(size_t)g].rc = r; sh[(size_t)g].done = true; }
      cv.notify_all();
    };
    auto collect_oldest = [&]() {
      const Fly f = fly[head];
      head = (head + 1) % ADSB_MAX_IN_FLIGHT; --n_fly;
      std::vector<adsb_burst> recs;
      const int r = collect_shard(c, f.ticket, &recs);
      if (r && !rc) rc = r;
      { std::lock_guard<std::mutex> lk(m); sh[(size_t)f.g].recs.swap(recs); }
      mark(f.g, r ? r : rc);
    };
    int g = g0;
    for (; g < g1 && !rc; ++g) {
      if (sh[(size_t)g].own_hi <= sh[(size_t)g].own_lo) { mark(g, 0); continue; }     // (a stream shorter than the tiling: nothing owned)
      if (n_fly == ADSB_MAX_IN_FLIGHT) collect_oldest();
      if (rc) break;
      int32_t ticket = -1;
      const int r = submit_shard_host(c, fmt, (const char*)host, sh[(size_t)g], n, kHeadFirst, &ticket);
      if (r) { rc = r; break; }
      fly[(head + n_fly) % ADSB_MAX_IN_FLIGHT] = Fly{g, ticket};
      ++n_fly;
    }
    while (n_fly > 0) collect_oldest();
    for (; g < g1; ++g) mark(g, rc ? rc : -EIO);                                     // what an error left unsubmitted
    feed_s[(size_t)k] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };

  for (int k = 0; k < n_ctx; ++k) {
    try {
      th.emplace_back(feeder, k);
    } catch (...) {
      // no thread for this context (resource limit): its shards fail, the others still run and are collected
      th.emplace_back();                                     // (keeps th[k] <-> context k; reserve() above: cannot throw)
      joined[(size_t)k] = 1;
      for (int g = k * shards_per_ctx; g < (k + 1) * shards_per_ctx; ++g) {
        { std::lock_guard<std::mutex> lk(m); sh[(size_t)g].rc = -ENOMEM; sh[(size_t)g].done = true; }
      }
      (void)fail(ctxs[k], -ENOMEM, "adsb_process_sharded_multi: could not start the feeder thread");
    }
  }
  auto join_one = [&](int k) { if (!joined[(size_t)k]) { if (th[(size_t)k].joinable()) th[(size_t)k].join(); joined[(size_t)k] = 1; } };

  // the calling thread: finished shards in stream order, head fix-up with the carried state, records to `out`
  SeamConsumer seam{sps, out, cap, abs_offset};
  int rc = 0;
  for (int g = 0; g < G; ++g) {
    MultiShard& S = sh[(size_t)g];
    {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return S.done; });
    }
    if (S.rc) { if (!rc) rc = S.rc; continue; }
    if (rc || S.own_hi <= S.own_lo) continue;
    adsb_ctx* c = ctxs[g / shards_per_ctx];
    // a head that ended inside a chain: this shard again on its own context, once its feeder is through with it
    auto rerun = [&](int head_cands, adsb_burst** rr, int32_t* nn) -> int {
      join_one(g / shards_per_ctx);
      int32_t ticket = -1;
      int e = submit_shard_host(c, fmt, (const char*)host, S, n, head_cands, &ticket);
      if (!e) e = collect_shard(c, ticket, &S.recs);
      *rr = S.recs.data(); *nn = (int32_t)S.recs.size();
      return e;
    };
    int32_t kept = 0;
    const int fb = seam.fallbacks;
    const int r = seam.take(S.recs.data(), (int32_t)S.recs.size(), rerun, &kept);
    if (r) { rc = r < 0 ? r : -EIO; if (r == -EAGAIN) rc = -EIO; continue; }
    c->stats.shard_fallbacks += seam.fallbacks - fb;
    std::vector<adsb_burst>().swap(S.recs);
  }
  for (int k = 0; k < n_ctx; ++k) join_one(k);
  if (stats) {
    stats->contexts = n_ctx; stats->shards = G; stats->fallbacks = seam.fallbacks;
    stats->wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    for (int k = 0; k < n_ctx; ++k) {
      stats->feeder_s[k] = feed_s[(size_t)k];
      stats->device[k] = ctxs[k]->device;
      stats->numa_node[k] = ctxs[k]->numa_node;
    }
  }
  if (rc) {
    for (int k = 0; k < n_ctx; ++k)
      if (ctxs[k] != c0 && ctxs[k]->err[0] && !c0->err[0]) snprintf(c0->err, sizeof(c0->err), "context %d: %s", k, ctxs[k]->err);
    return rc;
  }
  return seam.finish(n_out) ? fail(c0, -ENOSPC, "output array too small") : 0;
}

// ---- plain device memory for callers that do not link HIP (C / ctypes clients of the *_device entry points) ---------------
int adsb_device_alloc(adsb_ctx* c, void** d, size_t bytes) {
  if (!c || !d || bytes == 0) return -EINVAL;
  *d = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  if (hipMalloc(d, bytes) != hipSuccess) { (void)hipGetLastError(); *d = nullptr; return fail(c, -ENOMEM, "hipMalloc"); }
  return 0;
}

int adsb_device_free(adsb_ctx* c, void* d) {
  if (!c) return -EINVAL;
  if (!d) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipFree(d));
  return 0;
}

int adsb_device_upload(adsb_ctx* c, void* d, const void* host, size_t bytes) {
  if (!c || (bytes > 0 && (!d || !host))) return -EINVAL;
  if (bytes == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));      // blocking: the buffer is ready when this returns
  return 0;
}

// the host gates over delivered records: adsb_seam.h
int adsb_shard_fixup(adsb_burst* recs, int32_t n, int sps, int64_t eob_in, int32_t* n_kept) {
  if (n < 0 || (n > 0 && !recs) || sps < 2 || !n_kept) return -EINVAL;
  return shard_fixup(recs, n, sps, eob_in, n_kept);
}

int adsb_stitch(adsb_burst* cands, int32_t n, int sps, int32_t* n_kept) {
  if (n < 0 || (n > 0 && !cands) || sps < 2) return -EINVAL;
  return stitch(cands, n, sps, n_kept);
}

int adsb_host_alloc(void** p, size_t bytes) {
  if (!p || bytes == 0) return -EINVAL;
  *p = nullptr;
  return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess ? 0 : -ENOMEM;
}

int adsb_host_free(void* p) {
  if (!p) return 0;
  return hipHostFree(p) == hipSuccess ? 0 : -EINVAL;
}

int adsb_host_register(void* p, size_t bytes) {
  if (!p || bytes == 0) return -EINVAL;
  const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorHostMemoryAlreadyRegistered ? -EEXIST : -ENOMEM; }
  return 0;
}

int adsb_host_unregister(void* p) {
  if (!p) return -EINVAL;
  if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return -EINVAL; }
  return 0;
}

int adsb_get_stats(adsb_ctx* c, adsb_stats* out) {
  if (!c || !out) return -EINVAL;
  *out = c->stats;
  return 0;
}

int adsb_reset_stats(adsb_ctx* c) {
  if (!c) return -EINVAL;
  memset(&c->stats, 0, sizeof(c->stats));
  c->det_hist_n = 0;
  return 0;
}

int adsb_detect_history(adsb_ctx* c, float* ms, int32_t cap, int32_t* n) {
  if (!c || cap < 0 || (cap > 0 && !ms) || !n) return -EINVAL;
  const uint64_t have = c->det_hist_n < (uint64_t)adsb_ctx::kHist ? c->det_hist_n : (uint64_t)adsb_ctx::kHist;
  const uint64_t take = have < (uint64_t)cap ? have : (uint64_t)cap;
  for (uint64_t i = 0; i < take; ++i) ms[i] = c->det_hist[(c->det_hist_n - take + i) % adsb_ctx::kHist];   // oldest first
  *n = (int32_t)take;
  return 0;
}

const char* adsb_last_error(adsb_ctx* c) { return c ? c->err : "null context"; }

}  // extern "C"
