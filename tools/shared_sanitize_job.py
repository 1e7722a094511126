"""Write the job file of tests/sim/shared_sanitize_main.cpp: the calls of tests/golden/g_shared.npz (partition 0) under
("All Messages", "Conservative") and what the plain-Python replays expect of them.  tools/shared_sanitize.sh runs it."""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shared_replay as T                # noqa: E402


def main(path):
    g = np.load(T.GOLD)
    filt, corr = "All Messages", "Conservative"
    rep = T.Replay(filt, corr)
    calls = T.golden_calls(g, 0)
    with open(path, "wb") as f:
        f.write(struct.pack("<iiid", 4, 1, 1, float(g["fs"])) + g["start"].astype("<f8").tobytes() + struct.pack("<i", len(calls)))
        for idx, extra in calls:
            stream = g["stream"][idx]
            cut = np.concatenate([[0], np.flatnonzero(np.diff(stream)) + 1])
            items = [(int(stream[c]), int(c)) for c in cut]
            for k, s in extra:
                items.insert(k, (s, items[k][1] if k < len(items) else len(idx)))
            flags, rows, order = rep.call(g["bits"][idx], g["ts"][idx])
            f.write(struct.pack("<ii", len(idx), len(items)))
            f.write(np.array([s for s, _ in items], "<i4").tobytes() + np.array([c for _, c in items] + [len(idx)], "<i4").tobytes())
            f.write(np.ascontiguousarray(g["bits"][idx]).tobytes() + g["offset"][idx].astype("<i8").tobytes())
            f.write(flags.astype("<u2").tobytes() + T.rows_of(rows).tobytes() + order.astype("<i4").tobytes())


if __name__ == "__main__":
    main(sys.argv[1])
