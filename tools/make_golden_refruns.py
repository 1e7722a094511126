"""Container-only: record tests/golden/ref_runs.npz and tests/golden/ref_grc_digests.json -- the reference's outputs for
the exact inputs the reference-pinning tests hand it (tests/refstore.py).  Runs those tests with the UNMODIFIED reference
(tools/ref_harness.py) behind refstore.harness() and files every answer under the digest of its input.  Data only: the
reference's outputs, and sha256 digests of its GRC descriptors' fields (never their text).

    python tools/make_golden_refruns.py <gr-adsb checkout>
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import pytest              # noqa: E402
import yaml                # noqa: E402
import ref_harness         # noqa: E402
import refstore            # noqa: E402

# (test_packaging first: its GNU Radio stand-in must be in place before ref_harness installs its own)
TESTS = ["tests/test_packaging.py", "tests/test_oracle_vs_reference.py",
         "tests/test_ref_structured.py::test_against_the_real_reference", "tests/test_decoder_witness.py"]
GRC_FILES = ("adsb_framer.block.yml", "adsb_demod.block.yml")
GRC_KEYS = ("id", "templates", "parameters", "inputs", "outputs", "file_format", "label", "category")


class Recorder:
    """refstore.Stored's interface, answered by the live reference; keeps every answer for the store."""

    def __init__(self, ref_dir):
        self.ref_dir = ref_dir
        self.runs, self.parity, self.decodes = {}, {}, {}

    def run_reference(self, x, fs, threshold, schedule=None):
        r = ref_harness.run_reference(x, fs, threshold, schedule)
        r["pdu_conf_sha256"] = refstore.conf_digest(r["pdu_conf"])
        self.runs[refstore.run_key(x, fs, threshold, schedule)] = r
        return r

    def header_parity(self, bits, add_to_table):
        dec = ref_harness.load_reference_decoder("All Messages", "None", "None")
        res = {f: np.zeros(len(bits), np.int64) for f in refstore.PARITY_FIELDS}
        for i, b in enumerate(bits):
            dec.reset(); dec.bits = b.astype(int); dec.datetime = ""; dec.snr = 0.0; dec.timestamp = 0.0
            dec.decode_header()
            res["passed"][i] = dec.check_parity()
            res["df"][i], res["payload_length"][i] = dec.df, dec.payload_length
            aa = getattr(dec, "aa", None)
            res["aa"][i] = aa if isinstance(aa, (int, np.integer)) else -1
            res["in_table"][i] = getattr(dec, "aa_str", None) in dec.plane_dict
            if add_to_table[i]:
                dec.plane_dict[dec.aa_str] = {"callsign": ""}
        self.parity[refstore.parity_key(bits, add_to_table)] = res
        return res

    def decode_all(self, pdus):
        dec = ref_harness.load_reference_decoder()
        errors = []
        for i, p in enumerate(pdus):
            try:
                dec.decode_packet(p)
            except Exception as e:        # random payloads reach unfinished branches of the reference decoder
                errors.append((i, type(e).__name__, str(e)))
        dec.msgs.append(("errors", errors, None))
        msgs = [(port, repr(m)) for port, m, _ in dec.msgs]
        planes = {k: repr(sorted(v.items())) if isinstance(v, dict) else repr(v) for k, v in dec.plane_dict.items()}
        s = json.dumps({"msgs": msgs, "planes": planes})
        self.decodes[refstore.decode_key(pdus)] = s
        s = json.loads(s)
        return [tuple(m) for m in s["msgs"]], s["planes"]

    def grc_digests(self):
        out = {}
        for name in GRC_FILES:
            with open(os.path.join(self.ref_dir, "grc", name)) as f:
                d = yaml.safe_load(f)
            out[name] = {k: refstore.grc_digest(d[k]) for k in GRC_KEYS}
        return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.abspath(sys.argv[1])
    ref_harness.REF = os.path.join(ref_dir, "python", "adsb")
    rec = refstore.ACTIVE = Recorder(ref_dir)
    os.chdir(ROOT)
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + TESTS)
    if rc != 0:
        sys.exit("the tests failed against the live reference: nothing written")
    np.savez_compressed(refstore.RUNS, **refstore.pack(rec.runs, rec.parity, rec.decodes))
    with open(refstore.GRC_DIGESTS, "w") as f:
        json.dump(rec.grc_digests(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(refstore.RUNS, "%d streams, %d parity sets, %d decoder runs:" % (len(rec.runs), len(rec.parity), len(rec.decodes)),
          os.path.getsize(refstore.RUNS), "bytes;", refstore.GRC_DIGESTS)


if __name__ == "__main__":
    main()
