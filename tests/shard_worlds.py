"""Matched-centre lists cut into shards, for the host-only seam tests (test_shard_stitch_property.py, test_seam.py): what a
shard pass delivers, stated by its definition, the one sequential gate over the whole list, and the worlds both tests draw."""
import numpy as np
from hypothesis import strategies as st

from gr_adsb_amd import _native as N


def device_shard(offs, long_hint, sps, head_n):
    """What adsb_shard_device(head_cands=head_n) returns for a shard whose matched centres are `offs`: the gate run
    from fresh state (KEPT), the first head_n centres delivered whether kept or not (HEAD)."""
    n = len(offs)
    gate = np.where(long_hint, 119, 63) * sps
    kept = np.zeros(n, dtype=bool)
    eob = -(1 << 61)
    for i in range(n):
        if offs[i] > eob:
            kept[i] = True
            eob = int(offs[i]) + int(gate[i])
    head = np.arange(n) < head_n
    sel = kept | head
    recs = np.zeros(int(sel.sum()), dtype=N.BURST_DTYPE)
    recs["offset"] = offs[sel]
    recs["flags"] = (np.where(kept[sel], N.BURST_KEPT, 0) | np.where(head[sel], N.BURST_HEAD, 0)
                     | np.where(long_hint[sel], N.BURST_LONG_HINT, 0)).astype(np.uint16)
    return recs


def ungated_shard(offs, long_hint):
    recs = np.zeros(len(offs), dtype=N.BURST_DTYPE)
    recs["offset"] = offs
    recs["flags"] = np.where(long_hint, N.BURST_LONG_HINT, 0).astype(np.uint16)
    return recs


def truth(offs, long_hint, sps):
    c = ungated_shard(offs, long_hint)
    return N.stitch(c, sps)


def partition(offs, cuts):
    """Owner ranges (cuts = sorted stream offsets where a new shard begins) -> one mask over `offs` per shard."""
    edges = [-(1 << 60)] + list(cuts) + [1 << 60]
    return [(offs >= lo) & (offs < hi) for lo, hi in zip(edges[:-1], edges[1:])]


@st.composite
def worlds(draw):
    sps = draw(st.sampled_from([2, 4, 8, 20]))
    gate = 63 * sps
    n = draw(st.integers(0, 60))
    # gaps around the two gate windows, so that chains, chain breaks and exact ties all occur
    gaps = draw(st.lists(st.one_of(st.integers(1, 3), st.integers(gate - 2, gate + 2), st.integers(119 * sps - 2, 119 * sps + 2),
                                   st.integers(1, 3 * gate)), min_size=n, max_size=n))
    offs = np.cumsum(np.asarray(gaps, dtype=np.int64)) + 1000 if n else np.zeros(0, dtype=np.int64)
    long_hint = np.asarray(draw(st.lists(st.booleans(), min_size=n, max_size=n)), dtype=bool) if draw(st.booleans()) \
        else np.zeros(n, dtype=bool)
    hi = int(offs[-1]) + 10 if n else 2000
    # shard boundaries anywhere, including shards one sample long
    ncut = draw(st.integers(0, 12))
    cuts = sorted(set(draw(st.lists(st.integers(990, hi), min_size=ncut, max_size=ncut))))
    head_n = draw(st.sampled_from([1, 2, 3, 8, 64]))
    return offs, long_hint, cuts, sps, head_n
