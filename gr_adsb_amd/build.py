"""Build libadsb_hip.so (gfx950) in-tree with hipcc.  `python -m gr_adsb_amd.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libadsb_hip.so")
SOURCES = ["adsb_hip.hip"]
# ADSB_FLAG_STREAM_DECODE_SHARED's kernels: a translation unit of its own, so that adsb_hip.hip's kernels compile as without it
SHARED_SOURCE = "adsb_shared.hip"
# ADSB_FLAG_STREAM_DEDUP's kernels: a third unit, for the same reason
DEDUP_SOURCE = "adsb_dedup.hip"
# adsb_stream_mlat's kernels: a fourth unit, for the same reason
MLAT_SOURCE = "adsb_mlat.hip"
# adsb_stream_mlat_rule's kernels (the damped solver): a fifth unit, for the same reason
MLAT_RULE_SOURCE = "adsb_mlat_rule.hip"
# the MLAT track store's kernels (adsb_stream_mlat_track, the readout and expiry): a sixth unit, for the same reason
MLAT_TRACK_SOURCE = "adsb_mlat_track.hip"
# ADSB_FLAG_FEC_SOFT's kernels (the soft-decision CRC repair) and the rule's host form: a seventh unit, for the same reason
SOFTFEC_SOURCE = "adsb_softfec.hip"
# ADSB_FLAG_FEC_SOFT_BATCH's kernel (the same repair on a batch pass's packed list): an eighth unit, for the same reason
SOFTFEC_BATCH_SOURCE = "adsb_softfec_batch.hip"
DEPS = ["adsb_hip.hip", "adsb_env_hip.h", "adsb_device.h", "adsb_reply_device.h", "adsb_plan.h", "adsb_seam.h", os.path.join("..", "..", "include", "adsb_hip.h"),
        "adsb_shared.hip", "adsb_shared.h", "adsb_shared_device.h", "adsb_dedup.hip", "adsb_dedup.h", "adsb_dedup_device.h",
        "adsb_mlat.hip", "adsb_mlat.h", "adsb_mlat_device.h",
        "adsb_mlat_rule.hip", "adsb_mlat_rule.h", "adsb_mlat_rule_device.h",
        "adsb_mlat_track.hip", "adsb_mlat_track.h", "adsb_mlat_track_device.h",
        "adsb_softfec.hip", "adsb_softfec.h", "adsb_softfec_device.h",
        "adsb_softfec_batch.hip", "adsb_softfec_batch.h", "adsb_softfec_batch_device.h"]
# -ffp-contract=off: |IQ|^2 must be two rounded products and one rounded add
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def up_to_date():
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(os.path.join(CSRC, d)) <= t for d in DEPS)


RES = os.path.join(HERE, "kernel_resources.json")
RES_SHARED = os.path.join(HERE, "kernel_resources_shared.json")
RES_DEDUP = os.path.join(HERE, "kernel_resources_dedup.json")
RES_MLAT = os.path.join(HERE, "kernel_resources_mlat.json")
RES_MLAT_RULE = os.path.join(HERE, "kernel_resources_mlat_rule.json")
RES_MLAT_TRACK = os.path.join(HERE, "kernel_resources_mlat_track.json")
RES_SOFTFEC = os.path.join(HERE, "kernel_resources_softfec.json")
RES_SOFTFEC_BATCH = os.path.join(HERE, "kernel_resources_softfec_batch.json")
ALL_RES = (RES, RES_SHARED, RES_DEDUP, RES_MLAT, RES_MLAT_RULE, RES_MLAT_TRACK, RES_SOFTFEC, RES_SOFTFEC_BATCH)


def _parse_resources(remarks):
    """-Rpass-analysis=kernel-resource-usage remarks -> {kernel: {vgprs, sgprs, scratch, lds, occupancy, ...}}."""
    import re
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
            "LDS Size [bytes/block]": "lds_bytes_per_block"}
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+?): (\d+)", line)
        if m and cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return out


def compile_and_link(out, extra_flags=(), verbose=False):
    """The translation units, each compiled with FLAGS + extra_flags side by side, linked into the shared library `out`
    (libadsb_hip.so, or a side copy: tools/kbench.py) -> [the compiler's output per unit: SOURCES, SHARED_SOURCE, DEDUP_SOURCE, MLAT_SOURCE,
    MLAT_RULE_SOURCE, MLAT_TRACK_SOURCE, SOFTFEC_SOURCE, SOFTFEC_BATCH_SOURCE].  The objects live
    in a temporary directory."""
    import shutil
    import tempfile
    compile_flags = [f for f in FLAGS if f != "-shared"] + list(extra_flags)
    tmp = tempfile.mkdtemp(prefix="adsb_build_")
    try:
        units = [(os.path.join(CSRC, s), os.path.join(tmp, s + ".o")) for s in SOURCES + [SHARED_SOURCE, DEDUP_SOURCE, MLAT_SOURCE, MLAT_RULE_SOURCE, MLAT_TRACK_SOURCE,
                                                                                                  SOFTFEC_SOURCE, SOFTFEC_BATCH_SOURCE]]
        jobs = []
        for src, obj in units:
            cmd = [hipcc()] + compile_flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        outs = [(cmd, p.communicate()[0], p.returncode) for cmd, p in jobs]
        for cmd, text, rc in outs:
            if rc != 0:
                sys.stderr.write(text)
                raise subprocess.CalledProcessError(rc, cmd)
        cmd = [hipcc()] + FLAGS + list(extra_flags) + [obj for _, obj in units] + ["-o", out]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            raise subprocess.CalledProcessError(r.returncode, cmd)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return [text for _, text, _ in outs]


def build(force=False, verbose=False):
    """hipcc -> libadsb_hip.so, and beside it kernel_resources.json: the compiler's per-kernel register / LDS / scratch
    report (tests/test_abi.py holds the limits the pipeline relies on: k_detect must leave the tail kernels room), and
    kernel_resources_shared.json / kernel_resources_dedup.json / kernel_resources_mlat.json / kernel_resources_mlat_rule.json /
    kernel_resources_mlat_track.json / kernel_resources_softfec.json / kernel_resources_softfec_batch.json: the same for adsb_shared.hip's,
    adsb_dedup.hip's, adsb_mlat.hip's, adsb_mlat_rule.hip's, adsb_mlat_track.hip's, adsb_softfec.hip's and adsb_softfec_batch.hip's kernels."""
    if not force and up_to_date() and all(os.path.exists(p) for p in ALL_RES):
        return LIB
    import json
    remarks = compile_and_link(LIB, verbose=verbose)
    assert len(SOURCES) == 1
    for path, text in zip(ALL_RES, remarks):
        with open(path, "w") as f:
            json.dump(_parse_resources(text), f, indent=1, sort_keys=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
