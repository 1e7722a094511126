"""The seam consumer of the two sharded drivers (gr_adsb_amd/csrc/adsb_seam.h: SeamConsumer -- fix-up, larger head, ungated
gate, carried end-of-burst state, append under cap) on the CPU, with a fake re-run in place of a device pass
(tests/sim/seam_driver.cpp): for ANY partition of ANY matched-centre list the consumer's output equals ONE sequential gate
over all centres (adsb_stitch).  A shard pass is replaced by its definition (shard_worlds.device_shard).  The first head is
1..3 centres and a list with a head of 4 or 8 stands in for the largest head, so that shards of a few centres reach all three
outcomes: synchronised at once, synchronised with the second head, ungated."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings, strategies as st

from gr_adsb_amd import _native as N
from shard_worlds import device_shard, partition, truth, ungated_shard, worlds

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "sim")
SEAM_SO = os.path.join(SIM_DIR, "libadsb_seam_sim.so")
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    N.load()
    csrc = os.path.join(HERE, "..", "gr_adsb_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, "seam_driver.cpp"), os.path.join(csrc, "adsb_seam.h"), os.path.join(csrc, "adsb_plan.h"),
            os.path.join(HERE, "..", "include", "adsb_hip.h")]
    if not (os.path.exists(SEAM_SO) and all(os.path.getmtime(SEAM_SO) >= os.path.getmtime(s) for s in srcs)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               srcs[0], "-o", SEAM_SO])
    so = ctypes.CDLL(SEAM_SO)
    assert so.seam_head_first() == 64 and so.seam_head_max() == N.MAX_HEAD == 4096
    return so


def shards_of(offs, long_hint, cuts, sps, h1, h2):
    """every shard as its three lists: delivered with head h1, with head h2, ungated"""
    return [(device_shard(offs[m], long_hint[m], sps, h1), device_shard(offs[m], long_hint[m], sps, h2),
             ungated_shard(offs[m], long_hint[m])) for m in partition(offs, cuts)]


def consume(lib, shards, sps, cap, abs_offset=0, fail=(-1, 0, 0)):
    """seam_run -> (rc, the array given as `out` whole, cap, total, eob, fallbacks, n_out, finish_rc, outcomes)"""
    lists = [l for s in shards for l in s]
    start = np.zeros(len(lists) + 1, dtype=np.int64)
    start[1:] = np.cumsum([len(l) for l in lists])
    recs = np.concatenate(lists) if lists else np.zeros(0, dtype=N.BURST_DTYPE)
    out = np.zeros(cap + 4, dtype=N.BURST_DTYPE)             # four records of room behind cap: nothing may land there
    out["offset"] = -7
    total, eob = ctypes.c_int64(0), ctypes.c_int64(0)
    fb, n_out, frc = ctypes.c_int(0), ctypes.c_int32(0), ctypes.c_int(0)
    outcome = np.zeros(max(1, len(shards)), dtype=np.int32)
    rc = lib.seam_run(vp(recs.ctypes.data), vp(start.ctypes.data), len(shards), int(sps), ctypes.c_int64(abs_offset), vp(out.ctypes.data),
                      ctypes.c_int32(cap), int(fail[0]), int(fail[1]), int(fail[2]), ctypes.byref(total), ctypes.byref(eob), ctypes.byref(fb),
                      ctypes.byref(n_out), ctypes.byref(frc), vp(outcome.ctypes.data))
    return rc, out, total.value, eob.value, fb.value, n_out.value, frc.value, outcome[:len(shards)].tolist()


def test_any_partition_equals_one_sequential_gate(lib):
    seen = set()

    @seed(20261020)
    @settings(max_examples=400, deadline=None, database=None, suppress_health_check=[HealthCheck.too_slow])
    @given(worlds(), st.sampled_from([1, 2, 3]), st.sampled_from([4, 8]), st.sampled_from([0, 12345, -999, 1 << 40]))
    def run(w, h1, h2, abs_offset):
        offs, long_hint, cuts, sps, _ = w
        shards = shards_of(offs, long_hint, cuts, sps, h1, h2)
        want = truth(offs, long_hint, sps)
        nk = len(want)
        for cap in sorted({0, max(0, nk - 1), nk}):
            rc, out, total, eob, fb, n_out, frc, outcome = consume(lib, shards, sps, cap, abs_offset)
            assert rc == 0 and total == nk == n_out                  # the number kept, whether there was room or not
            assert fb == sum(o > 0 for o in outcome) and all(o in (0, 1, 2) for o in outcome)
            assert eob == (int(want["offset"][-1]) + int(N.gate_window(want[-1:], sps)[0]) if nk else -(1 << 60))
            assert frc == (-errno.ENOSPC if nk > cap else 0)
            assert np.all(out["offset"][cap:] == -7) and not out["flags"][cap:].any()      # nothing beyond cap
            if frc == 0:
                got = out[:nk]
                assert np.all(got["flags"] & N.BURST_KEPT) and not np.any(got["flags"] & N.BURST_HEAD)
                # abs_offset is added to the offsets and to nothing else
                shifted = want.copy()
                shifted["offset"] += abs_offset
                assert got.tobytes() == shifted.tobytes()
            seen.update(outcome)

    run()
    assert seen == {0, 1, 2}, seen         # synchronised at once, with the second head, ungated: each occurred


def test_the_three_outcomes_by_hand(lib):
    """sps 2 (window 126).  Shard 1 = a chain 1010, 1090, 1170, 1250 behind a record at 950 (eob 1076), then 2000 on its own:
    a head of 5 reaches the centre that starts an independent chain, a head of 1 or 2 ends inside the chain."""
    lh = np.zeros(6, dtype=bool)
    offs = np.array([950, 1010, 1090, 1170, 1250, 2000], dtype=np.int64)
    want = truth(offs, lh, 2)["offset"].tolist()
    assert want == [950, 1090, 1250, 2000]
    for h1, h2, outcome in ((5, 8, 0), (1, 5, 1), (1, 2, 2)):
        rc, out, total, eob, fb, n_out, frc, oc = consume(lib, shards_of(offs, lh, [1000], 2, h1, h2), 2, 8)
        assert (rc, frc, total, n_out) == (0, 0, 4, 4) and out["offset"][:4].tolist() == want
        assert oc == [0, outcome] and fb == (outcome > 0) and eob == 2000 + 126
    # a list that is all head and ends inside the chain it began in: whether its pass's head was full the list cannot say
    # (1128 lies behind 1002's window from fresh state, but not behind 1001's), so the shard is run again
    offs = np.array([1001, 1002, 1003, 1004, 1128], dtype=np.int64)
    rc, out, total, eob, fb, n_out, frc, oc = consume(lib, shards_of(offs, lh[:5], [1002], 2, 1, 4), 2, 8)
    assert (rc, total) == (0, 2) and out["offset"][:2].tolist() == [1001, 1128] == truth(offs, lh[:5], 2)["offset"].tolist()
    assert oc == [0, 2]


@pytest.mark.parametrize("fail_head,code", [(4096, -5), (0, -75), (4096, 3)])
def test_a_failed_rerun_ends_take_with_its_code_and_moves_nothing(lib, fail_head, code):
    lh = np.zeros(6, dtype=bool)
    offs = np.array([950, 1010, 1090, 1170, 1250, 2000], dtype=np.int64)
    shards = shards_of(offs, lh, [1000, 1900], 2, 1, 2)         # shard 1 goes all the way to the ungated step
    before = consume(lib, shards[:1], 2, 8)
    assert before[0] == 0 and before[2] == 1
    rc, out, total, eob, fb, n_out, frc, oc = consume(lib, shards, 2, 8, fail=(1, fail_head, code))
    assert rc == code and oc == [0, -1, -1]
    assert (total, eob, fb) == (before[2], before[3], 0) == (1, 950 + 126, 0)      # as they were before the call
    assert out["offset"][:1].tolist() == [950] and np.all(out["offset"][1:] == -7)  # that shard appended nothing
