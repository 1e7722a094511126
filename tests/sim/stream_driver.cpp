// stream_driver.cpp -- TEST INFRASTRUCTURE ONLY.  The stream-batch path of the library (adsb_process_stream_batch*:
// k_stream_stage, k_batch, k_batch_pack, k_stream_save) compiled against the SIMT emulator in hipsim.h and run on host memory,
// with the plan, the copy tables and the delivery rule of adsb_plan.h the library itself uses (plan_stream_item,
// fill_stream_copies, stream_deliver).  A handle is a set of streams of one format and rate: their positions, carried
// end-of-burst offsets, bases, overlong counts and two carry slots each.  There is no host fallback here: an item the kernel
// could not finish is reported (kept[i] = -1) and its stream does not move.
// Built by tests/test_stream_batch.py; never linked into libadsb_hip.so.
#include "hipsim.h"

#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_device.h"
#include "../../gr_adsb_amd/csrc/adsb_plan.h"

using namespace adsb;

namespace {

struct SimStream {
  long long pos = 0, eob = kStreamFreshEob, base = 0, overlong = 0;
  int cur = 0;                          // the carry slot that holds the stream's last samples
};
struct SimStreams {
  int mode = 0, sps = 2, bps = 8, long_aware = 0;
  float scale = 1.0f;
  size_t slot_bytes = 0;                // one carry slot (a multiple of 256 bytes)
  std::vector<SimStream> st;
  char* carry = nullptr;                // [n_streams][2][slot_bytes]
  char* slot(int id, int which) const { return carry + ((size_t)id * 2 + (size_t)which) * slot_bytes; }
};

template <int MODE>
void run_k_batch(int sps, int n_items, const DetectArgs* da, const TailArgs* ta, int* kept) {
  if (sps == 2) hipsim::launch(k_batch<MODE, 1>, (unsigned)n_items, kThreads, da, ta, kept);
  else hipsim::launch(k_batch<MODE, 0>, (unsigned)n_items, kThreads, da, ta, kept);
}

}  // namespace

extern "C" {

void* stream_open(int mode, int sps, int n_streams, float scale, int long_aware) {
  if (mode < 0 || mode > 4 || sps < 2 || n_streams < 1) return nullptr;
  SimStreams* h = new SimStreams;
  h->mode = mode; h->sps = sps; h->bps = mode_bytes(mode); h->scale = scale; h->long_aware = long_aware;
  h->slot_bytes = ((size_t)stream_carry_max(sps) * (size_t)h->bps + 255) & ~(size_t)255;
  h->st.resize((size_t)n_streams);
  h->carry = (char*)aligned_alloc(256, (size_t)n_streams * 2 * h->slot_bytes);
  memset(h->carry, 0x5A, (size_t)n_streams * 2 * h->slot_bytes);
  return h;
}
void stream_close(void* hv) {
  SimStreams* h = (SimStreams*)hv;
  free(h->carry);
  delete h;
}
int stream_set_base(void* hv, int id, long long base) {
  SimStreams* h = (SimStreams*)hv;
  if (id < 0 || id >= (int)h->st.size() || h->st[(size_t)id].pos != 0) return -1;
  h->st[(size_t)id].base = base;
  return 0;
}
int stream_state(void* hv, int id, long long* pos, long long* eob, long long* overlong) {
  SimStreams* h = (SimStreams*)hv;
  if (id < 0 || id >= (int)h->st.size()) return -1;
  const SimStream& s = h->st[(size_t)id];
  *pos = s.pos; *eob = s.eob; *overlong = s.overlong;
  return 0;
}
// the stream's carry as it lies in its current slot -> bytes copied (the whole slot's capacity is cap_bytes at least)
long long stream_carry(void* hv, int id, void* out, long long cap_bytes) {
  SimStreams* h = (SimStreams*)hv;
  if (id < 0 || id >= (int)h->st.size()) return -1;
  const SimStream& s = h->st[(size_t)id];
  const long long bytes = stream_carry_len(s.pos, h->sps) * h->bps;
  if (bytes > cap_bytes) return -2;
  memcpy(out, h->slot(id, s.cur), (size_t)bytes);
  return bytes;
}
long long stream_carry_max_samples(int sps) { return stream_carry_max(sps); }
// plan_stream_item's fields, for the test that restates them: out[13]
void stream_plan(long long pos, long long n, int end, long long base, long long eob, int sps, long long* out) {
  const StreamItem it = plan_stream_item(1, pos, n, end != 0, base, eob, sps);
  const Plan& p = it.plan;
  const long long v[13] = {p.origin, p.n, p.in0_base, p.scan_lo, p.scan_hi, p.fall_hi, p.dem_hi, p.end_is_call_end,
                           p.prev_eob_stream, p.gate ? 1 : 0, p.head_n, it.run ? 1 : 0, it.origin};
  for (int k = 0; k < 13; ++k) out[k] = v[k];
}

// One call: item i appends n[i] samples at data[i] (any sample-aligned address) to stream ids[i]; end[i] != 0: the END item.
// device_entry != 0: k_stream_stage copies the chunks (the device entry point); else they are put in place by memcpy as the
// host entry point's upload does.  rec_cap_in > 0 replaces the product's list capacity.  out: out_cap records; item_first
// [n_items + 1]; kept[n_items] (k_batch's verdict); sumflags[n_items] (k_stream_save's status word).  Returns the number of
// delivered records, or < 0.
int stream_push(void* hv, int n_items, const int* ids, const void* const* data, const long long* n, const int* end,
                const float* thr, int rec_cap_in, int device_entry, unsigned long long* out, int out_cap, int* item_first,
                int* kept_out, unsigned* sumflags) {
  SimStreams* h = (SimStreams*)hv;
  if (n_items < 1) return -2;
  const int sps = h->sps, bps = h->bps;
  std::vector<char> seen(h->st.size(), 0);
  for (int i = 0; i < n_items; ++i) {
    if (ids[i] < 0 || ids[i] >= (int)h->st.size() || seen[(size_t)ids[i]] || n[i] < 0) return -3;
    seen[(size_t)ids[i]] = 1;
  }
  // the staging buffer: every item on a 256-byte boundary, filled with 0xA5 bytes (the library does not clear it either)
  std::vector<StreamItem> plan((size_t)n_items);
  std::vector<size_t> off((size_t)n_items);
  size_t stage_bytes = 0;
  for (int i = 0; i < n_items; ++i) {
    const SimStream& s = h->st[(size_t)ids[i]];
    plan[(size_t)i] = plan_stream_item(h->mode, s.pos, n[i], end[i] != 0, s.base, s.eob, sps);
    off[(size_t)i] = stage_bytes;
    stage_bytes += ((size_t)plan[(size_t)i].n_buf * (size_t)bps + 255) & ~(size_t)255;
  }
  char* stage = (char*)aligned_alloc(256, stage_bytes + 256);
  memset(stage, 0xA5, stage_bytes + 256);
  std::vector<StreamStage> sg((size_t)n_items);
  std::vector<StreamSave> sv((size_t)n_items);
  for (int i = 0; i < n_items; ++i) {
    const SimStream& s = h->st[(size_t)ids[i]];
    fill_stream_copies(sg[(size_t)i], sv[(size_t)i], plan[(size_t)i], s.pos, n[i], sps, bps, stage + off[(size_t)i],
                       h->slot(ids[i], s.cur), h->slot(ids[i], s.cur ^ 1), device_entry ? data[i] : nullptr);
    if (!device_entry && n[i] > 0) memcpy(sg[(size_t)i].chunk.dst, data[i], (size_t)n[i] * (size_t)bps);
    plan[(size_t)i].plan.d_data = stage + off[(size_t)i];
    plan[(size_t)i].plan.long_aware = h->long_aware != 0;
  }
  hipsim::launch(k_stream_stage, (unsigned)n_items, kThreads, (const StreamStage*)sg.data());

  std::vector<BatchLay> lay((size_t)n_items);
  size_t total = 0;
  long long packed_cap = 0;
  const long long H = 8ll * sps;
  for (int i = 0; i < n_items; ++i) {
    const StreamItem& it = plan[(size_t)i];
    lay[(size_t)i].slots = 0;
    if (!it.run || it.n_buf > kBatchItemMax) continue;
    BatchGeom g = plan_batch_item(it.plan.scan_hi + (H - 1), sps, kWaves, kWTile);
    if (rec_cap_in > 0) g.rec_cap = rec_cap_in;
    lay[(size_t)i] = plan_batch_layout(total, g, kWaves, kThreads, sizeof(Rec), sizeof(LongRise));
    total = lay[(size_t)i].end;
    packed_cap += lay[(size_t)i].slots;
  }
  char* sc = (char*)aligned_alloc(128, total + 128);
  memset(sc, 0xA5, total + 128);
  std::vector<BatchFixed> fx((size_t)n_items);
  memset(fx.data(), 0, fx.size() * sizeof(BatchFixed));
  std::vector<DetectArgs> da((size_t)n_items);
  std::vector<TailArgs> ta((size_t)n_items);
  std::vector<int> kept((size_t)n_items, -7);
  memset(da.data(), 0, da.size() * sizeof(DetectArgs));
  memset(ta.data(), 0, ta.size() * sizeof(TailArgs));
  for (int i = 0; i < n_items; ++i) {
    if (lay[(size_t)i].slots == 0) { da[(size_t)i].n = plan[(size_t)i].run ? -1 : 0; continue; }
    fill_batch_item(da[(size_t)i], ta[(size_t)i], plan[(size_t)i].plan, lay[(size_t)i], sc, fx[(size_t)i], thr[i], h->scale, sps,
                    h->long_aware != 0, kWaves);
  }
  switch (h->mode) {
    case 0: run_k_batch<0>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 1: run_k_batch<1>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 2: run_k_batch<2>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 3: run_k_batch<3>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    default: run_k_batch<4>(sps, n_items, da.data(), ta.data(), kept.data()); break;
  }
  std::vector<Rec> packed((size_t)packed_cap + 1);
  std::vector<int> first((size_t)n_items + 1, -7), hkept((size_t)n_items, -7);
  Summary tot;
  memset(&tot, 0, sizeof(tot));
  hipsim::launch(k_batch_pack, (unsigned)n_items, kThreads, (const TailArgs*)ta.data(), (const int*)kept.data(), n_items,
                 packed.data(), (int)packed_cap, first.data(), hkept.data(), &tot, (Rec*)nullptr, 0);
  std::vector<StreamStatus> status((size_t)n_items);
  memset(status.data(), 0xEE, status.size() * sizeof(StreamStatus));
  hipsim::launch(k_stream_save, (unsigned)n_items, kThreads, (const StreamSave*)sv.data(), (const TailArgs*)ta.data(),
                 (const int*)kept.data(), status.data());
  // delivery and the streams' new state: adsb_plan.h's one rule
  int nres = 0, rc = 0;
  std::vector<Rec> keep;
  for (int i = 0; i < n_items && rc == 0; ++i) {
    item_first[i] = nres;
    kept_out[i] = kept[(size_t)i];
    sumflags[i] = status[(size_t)i].flags;
    if (status[(size_t)i].kept != kept[(size_t)i] || hkept[(size_t)i] != kept[(size_t)i]) { rc = -5; break; }
    if (kept[(size_t)i] < 0) continue;
    SimStream& s = h->st[(size_t)ids[i]];
    keep.resize((size_t)kept[(size_t)i] + 1);
    long long eob = s.eob, over = 0;
    const int w = stream_deliver(packed.data() + first[(size_t)i], kept[(size_t)i], keep.data(), plan[(size_t)i].plan,
                                 status[(size_t)i].flags, sps, [](const Rec& r) { return (long long)r.w[0]; },
                                 [](const Rec& r) { return (unsigned)(r.w[3] >> 48); }, &eob, &over);
    if (nres + w > out_cap) { rc = -1; break; }
    memcpy(out + 4 * (size_t)nres, keep.data(), (size_t)w * sizeof(Rec));
    nres += w;
    s.overlong += over;
    s.cur ^= 1;
    if (end[i]) { s.pos = 0; s.eob = kStreamFreshEob; }
    else { s.pos += n[i]; s.eob = eob; }
  }
  item_first[n_items] = nres;
  free(sc);
  free(stage);
  return rc ? rc : nres;
}
}
