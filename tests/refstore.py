"""The reference's own outputs for the exact inputs the reference-pinning tests hand it, stored as data under
tests/golden/ (ref_runs.npz, ref_grc_digests.json), so that those tests need nothing outside the repository.

harness() is what the tests call the reference through.  By default it serves the stored outputs: a call whose input is
not one the reference was run on has no stored answer and fails.  tools/make_golden_refruns.py records the store by
running the same tests with the live reference (tools/ref_harness.py) behind a Recorder."""
import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = os.path.join(GOLDEN_DIR, "ref_runs.npz")
GRC_DIGESTS = os.path.join(GOLDEN_DIR, "ref_grc_digests.json")
PARITY_FIELDS = ("df", "payload_length", "aa", "passed", "in_table")

ACTIVE = None          # a Recorder while tools/make_golden_refruns.py runs the tests; None: the stored outputs


def _update(h, p):
    if isinstance(p, np.ndarray):
        p = np.ascontiguousarray(p)
        h.update(("%s%r" % (p.dtype.str, p.shape)).encode())
        h.update(p.tobytes())
    elif isinstance(p, (list, tuple)):
        h.update(b"(%d" % len(p))
        for q in p:
            _update(h, q)
    elif isinstance(p, dict):
        for k in sorted(p):
            h.update(repr(k).encode())
            v = p[k]
            _update(h, np.asarray(v, dtype=np.float64) if np.isscalar(v) and not isinstance(v, str) else v)
    else:
        h.update(repr(p).encode())


def key(kind, *parts):
    """Digest of a call's full input: what a stored output is filed under."""
    h = hashlib.sha256(kind.encode())
    for p in parts:
        _update(h, p)
    return kind + "_" + h.hexdigest()[:24]


def run_key(x, fs, threshold, schedule):
    return key("run", np.ascontiguousarray(x, dtype=np.float32), np.float64(fs), np.float32(threshold),
               None if schedule is None else np.asarray(schedule, dtype=np.int64))


def parity_key(bits, add_to_table):
    return key("parity", np.asarray(bits, dtype=np.uint8), np.asarray(add_to_table, dtype=bool))


def decode_key(pdus):
    return key("decode", [(meta, np.asarray(vec, dtype=np.uint8)) for meta, vec in pdus])


def grc_digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def conf_digest(conf):
    """sha256 of demod.bit_confidence's ratios ([n,112] float32, bit for bit): the store keeps this instead of the 448
    bytes per PDU, and the tests compare the oracle's ratios through it -- still an exact comparison."""
    return hashlib.sha256(np.ascontiguousarray(conf, dtype="<f4").reshape(-1, 112).tobytes()).hexdigest()


# ---- the store's layout: one table per kind of call, the outputs of all calls concatenated (identical ones once) ----
TAG_COLS = (("tag_offsets", "<i8"), ("tag_snr", "<f4"))
PDU_COLS = (("pdu_offsets", "<i8"), ("pdu_bits", "u1"), ("pdu_snr", "<f4"))      # pdu_bits: 14 packed bytes per PDU


def _cols(r, cols):
    out = []
    for name, dt in cols:
        a = np.asarray(r[name])
        out.append(np.packbits(a.astype(np.uint8).reshape(-1, 112), axis=1) if name == "pdu_bits" else a.astype(dt))
    return out


class _Concat:
    """Runs of rows appended once per distinct content; ranges [lo, hi) into the concatenation."""

    def __init__(self, cols):
        self.cols, self.parts, self.n, self.seen = cols, [[] for _ in cols], 0, {}

    def add(self, arrays):
        k = key("rows", *arrays)
        if k not in self.seen:
            for part, a in zip(self.parts, arrays):
                part.append(a)
            self.seen[k] = (self.n, self.n + len(arrays[0]))
            self.n += len(arrays[0])
        return self.seen[k]

    def arrays(self):
        return {name: (np.concatenate(part) if part else np.zeros((0, 14) if name == "pdu_bits" else 0, dt))
                for (name, dt), part in zip(self.cols, self.parts)}


def pack(runs, parity, decodes):
    """{run key: run_reference's dict}, {parity key: header_parity's dict}, {decode key: JSON text} -> the arrays of
    ref_runs.npz (plain dtypes only: no pickled objects)."""
    tags, pdus = _Concat(TAG_COLS), _Concat(PDU_COLS)
    rk = sorted(runs)
    index = np.zeros((len(rk), 4), np.int64)
    eob, in0 = np.zeros(len(rk), np.int64), np.zeros(len(rk), np.float32)
    conf = np.zeros((len(rk), 32), np.uint8)
    for i, k in enumerate(rk):
        r = runs[k]
        index[i] = tags.add(_cols(r, TAG_COLS)) + pdus.add(_cols(r, PDU_COLS))
        eob[i], in0[i] = r["final_prev_eob"], r["final_prev_in0"]
        conf[i] = np.frombuffer(bytes.fromhex(r["pdu_conf_sha256"]), np.uint8)
    out = {"run_keys": np.array(rk, dtype="U"), "run_index": index, "run_final_prev_eob": eob, "run_final_prev_in0": in0,
           "run_pdu_conf_sha256": conf}
    out.update(tags.arrays())
    out.update(pdus.arrays())
    pk = sorted(parity)
    out["parity_keys"] = np.array(pk, dtype="U")
    out["parity_index"] = np.cumsum([0] + [len(parity[k]["df"]) for k in pk]).astype(np.int64)
    for f in PARITY_FIELDS:
        out["parity_" + f] = np.concatenate([np.asarray(parity[k][f], np.int64) for k in pk] or [np.zeros(0, np.int64)])
    dk = sorted(decodes)
    out["decode_keys"] = np.array(dk, dtype="U")
    out["decode_json"] = np.array([decodes[k] for k in dk], dtype="U")
    return out


class Stored:
    """Serves what the reference returned (tools/ref_harness.py's reductions of its outputs) for the stored inputs."""

    def __init__(self, path=RUNS):
        with np.load(path) as z:
            self.z = {name: z[name] for name in z.files}
        self.rows = {kind: {k: i for i, k in enumerate(self.z[kind + "_keys"].tolist())} for kind in ("run", "parity", "decode")}

    def _row(self, kind, k, what):
        if k not in self.rows[kind]:
            raise AssertionError("no stored reference output for this %s (%s): it is not the input the reference was run on "
                                 "(tools/make_golden_refruns.py records them)" % (what, k))
        return self.rows[kind][k]

    def run_reference(self, x, fs, threshold, schedule=None):
        """tools/ref_harness.run_reference: the framer's tags and the demod's PDUs for float32 |IQ|^2 x; the confidence
        ratios as their digest (pdu_conf_sha256, see conf_digest)."""
        z = self.z
        i = self._row("run", run_key(x, fs, threshold, schedule), "stream")
        t0, t1, p0, p1 = z["run_index"][i]
        out = {name: z[name][t0:t1] for name, _ in TAG_COLS}
        out.update((name, z[name][p0:p1]) for name, _ in PDU_COLS)
        out["pdu_bits"] = np.unpackbits(out["pdu_bits"], axis=1)[:, :112].reshape(-1, 112)
        out["final_prev_eob"] = int(z["run_final_prev_eob"][i])
        out["final_prev_in0"] = np.float32(z["run_final_prev_in0"][i])
        out["pdu_conf_sha256"] = z["run_pdu_conf_sha256"][i].tobytes().hex()
        return out

    def header_parity(self, bits, add_to_table):
        """The reference decoder's decode_header + check_parity on each row of bits (0/1, [n,112]) in turn, starting from an
        empty aircraft table; after row i with add_to_table[i] its announced address joins the table.  Per row: df,
        payload_length, aa, check_parity()'s return and whether aa was in the table when it was checked."""
        i = self._row("parity", parity_key(bits, add_to_table), "set of PDUs")
        lo, hi = self.z["parity_index"][i:i + 2]
        return {f: self.z["parity_" + f][lo:hi] for f in PARITY_FIELDS}

    def decode_all(self, pdus):
        """The reference decoder fed the PDUs in order: (messages it published, its aircraft table), as repr strings."""
        s = json.loads(str(self.z["decode_json"][self._row("decode", decode_key(pdus), "PDU list")]))
        return [tuple(m) for m in s["msgs"]], s["planes"]


_stored = []


def harness():
    if ACTIVE is not None:
        return ACTIVE
    if not _stored:
        _stored.append(Stored())
    return _stored[0]


def reference_grc_digests():
    """{descriptor file: {key: sha256 of the reference descriptor's value, canonical JSON}} (gr-adsb grc/*.block.yml)."""
    if ACTIVE is not None:
        return ACTIVE.grc_digests()
    with open(GRC_DIGESTS) as f:
        return json.load(f)
