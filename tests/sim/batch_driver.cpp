// batch_driver.cpp -- TEST INFRASTRUCTURE ONLY.  The batch path of the library (adsb_process_batch*: k_batch, one workgroup
// per item with its arguments from two tables, then k_batch_pack) compiled against the SIMT emulator in hipsim.h and run on
// host memory, with the item geometry of adsb_plan.h the library itself uses.  Items are read WHERE THEY LIE (no copy: a
// test that cuts neighbouring items out of one buffer checks that nothing of a neighbour is read).  There is no host
// fallback here: an item the kernel could not finish is reported (kept[i] = -1, overflow[i]) and contributes no records.
// Built by tests/test_batch.py; never linked into libadsb_hip.so.
#include "hipsim.h"

#include <vector>

#include "../../gr_adsb_amd/csrc/adsb_device.h"
#include "../../gr_adsb_amd/csrc/adsb_plan.h"

using namespace adsb;

template <int MODE>
static void run_k_batch(int sps, int n_items, const DetectArgs* da, const TailArgs* ta, int* kept) {
  // the instances the library launches (adsb_hip.hip: launch_batch): 2 Msps, and the run-time tap stride for every other rate
  if (sps == 2) hipsim::launch(k_batch<MODE, 1>, (unsigned)n_items, kThreads, da, ta, kept);
  else hipsim::launch(k_batch<MODE, 0>, (unsigned)n_items, kThreads, da, ta, kept);
}

extern "C" {

// mode = ADSB_FMT_*; data[i] 16-byte aligned, n[i] samples, read in place.  rec_cap_in > 0 replaces the product's list
// capacity for every item.  out: out_cap records of 4 words; item_first[n_items + 1]; kept[n_items] (k_batch's verdict: the
// item's record count or -1); overflow[n_items] (the item's Summary.overflow).  host_cap: records k_batch_pack also stores
// into host_out (the library's pinned head).  Returns the number of records, or < 0.
int batch_run(int mode, int sps, int n_items, const void* const* data, const long long* n, const long long* abs_offset,
              const float* thr, float scale, int rec_cap_in, int long_aware, unsigned long long* out, int out_cap,
              int* item_first, int* kept_out, int* overflow, unsigned long long* host_out, int host_cap) {
  if (n_items < 1) return -2;
  // the library's own layout and table fill (adsb_plan.h: plan_batch_layout, fill_batch_item), in ONE scratch buffer that is
  // filled with 0xA5 bytes first (the library does not clear it either); only the BatchFixed blocks start from zero
  std::vector<BatchLay> lay((size_t)n_items);
  size_t total = 0;
  long long packed_cap = 0;
  for (int i = 0; i < n_items; ++i) {
    if (((uintptr_t)data[i] & 15u) != 0 || n[i] < 0) return -3;
    lay[(size_t)i].slots = 0;
    if (n[i] == 0 || n[i] > kBatchItemMax) continue;
    BatchGeom g = plan_batch_item(n[i], sps, kWaves, kWTile);
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
    if (lay[(size_t)i].slots == 0) { da[(size_t)i].n = n[i] == 0 ? 0 : -1; continue; }
    fill_batch_item(da[(size_t)i], ta[(size_t)i], plan_canonical(mode, data[i], n[i], abs_offset[i], sps), lay[(size_t)i], sc,
                    fx[(size_t)i], thr[i], scale, sps, long_aware != 0, kWaves);
  }
  switch (mode) {
    case 0: run_k_batch<0>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 1: run_k_batch<1>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 2: run_k_batch<2>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 3: run_k_batch<3>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    case 4: run_k_batch<4>(sps, n_items, da.data(), ta.data(), kept.data()); break;
    default: return -4;
  }
  std::vector<Rec> packed((size_t)packed_cap + 1);
  std::vector<int> first((size_t)n_items + 1, -7), hkept((size_t)n_items, -7);
  Summary tot;
  memset(&tot, 0, sizeof(tot));
  hipsim::launch(k_batch_pack, (unsigned)n_items, kThreads, (const TailArgs*)ta.data(), (const int*)kept.data(), n_items,
                 packed.data(), (int)packed_cap, first.data(), hkept.data(), &tot, (Rec*)host_out, host_cap);
  for (int i = 0; i < n_items; ++i) {
    if (hkept[(size_t)i] != kept[(size_t)i]) return -5;
    item_first[i] = first[(size_t)i];
    kept_out[i] = kept[(size_t)i];
    overflow[i] = (n[i] == 0 || n[i] > kBatchItemMax) ? 0 : fx[(size_t)i].sum.overflow;
    // the long-pulse list is left empty for the scratch's next use
    if (n[i] > 0 && n[i] <= kBatchItemMax && (fx[(size_t)i].long_count != 0 || fx[(size_t)i].long_lastp != 0ull)) return -6;
  }
  item_first[n_items] = first[(size_t)n_items];
  const int nres = first[(size_t)n_items];
  if (tot.n_kept != nres) return -8;
  free(sc);
  if (nres > out_cap) return -1;
  memcpy(out, packed.data(), (size_t)nres * sizeof(Rec));
  return nres;
}

long long batch_item_max() { return kBatchItemMax; }
// the list capacity the library gives an item of n samples (slots per list; four lists per item)
int batch_rec_cap(long long n, int sps) { return plan_batch_item(n, sps, kWaves, kWTile).rec_cap; }
}
