// aircraft_driver.cpp -- TEST INFRASTRUCTURE ONLY.  Runs the product's aircraft-table kernels (gr_adsb_amd/csrc/adsb_device.h:
// k_air_announce, k_air_verdict, k_air_cond; ADSB_FLAG_AIRCRAFT_TABLE) on the SIMT emulator in hipsim.h, on host memory, in
// the order adsb_hip.hip's launch_air queues them.  Never linked into libadsb_hip.so.
#include "hipsim.h"

#include "../../gr_adsb_amd/csrc/adsb_device.h"

using namespace adsb;

extern "C" {

int sim_air_state_bytes() { return (int)sizeof(AirState); }

// one pass over a delivered list: recs = n records of 4 words, flagged in place; mirror (may be null): the pinned copy of
// the first mirror_cap records; table = 2^24 keys; st = an AirState; pass = the pass number
int sim_air_pass(unsigned long long* recs, int n, int grid, unsigned long long* mirror, int mirror_cap, unsigned long long* table,
                 void* st, unsigned long long pass, int fec) {
  Summary sum{};
  sum.n_kept = n;
  AirArgs a{};
  a.out = (Rec*)recs; a.mirror = (Rec*)mirror; a.mirror_cap = mirror ? mirror_cap : 0;
  a.sum = &sum; a.cap = n; a.host_sum = &sum; a.table = table; a.st = (AirState*)st; a.pass = pass << 32; a.fec = fec;
  hipsim::launch(k_air_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_air_cond, 1u, 64u, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  return (int)(sum.flags >> 31);
}

// the same over adsb_demod_work's slices (bits14 / ok)
int sim_air_slices(unsigned char* bits14, unsigned char* ok, int ntags, int grid, unsigned long long* table, void* st,
                   unsigned long long pass, int fec) {
  AirArgs a{};
  a.bits14 = bits14; a.ok = ok; a.cap = ntags; a.table = table; a.st = (AirState*)st; a.pass = pass << 32; a.fec = fec;
  hipsim::launch(k_air_announce, (unsigned)grid, (unsigned)kThreads, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 0);
  hipsim::launch(k_air_cond, 1u, 64u, a);
  hipsim::launch(k_air_verdict, (unsigned)grid, (unsigned)kThreads, a, 1);
  return 0;
}
}
