"""How tests/test_gpu_shared_device.py and tests/test_gpu_dedup_device.py build their device libraries, the way
test_gpu_mlat_device.device_lib does: the SHIPPED translation unit compiled with exactly the library's flags as one unit, the
driver under tests/gpu/ as a second with -Wall -Wextra, each in a hipcc process of its own, linked side by side.  Test
infrastructure only."""
import os
import shutil
import subprocess
import tempfile
import time

from gr_adsb_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
DEV_DIR = os.path.join(HERE, "gpu")


def device_lib(unit, driver, so_name, deps):
    """unit: a source of gr_adsb_amd/csrc; driver: a source of tests/gpu; deps: further files of csrc the two include
    -> the path of tests/gpu/<so_name>, rebuilt where a source is newer"""
    src, drv, so = os.path.join(B.CSRC, unit), os.path.join(DEV_DIR, driver), os.path.join(DEV_DIR, so_name)
    srcs = [src, drv, os.path.join(DEV_DIR, "device_buffers.h")] + [os.path.join(B.CSRC, f) for f in deps]
    if os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(s) for s in srcs):
        return so
    t0 = time.time()
    compile_flags = [f for f in B.FLAGS if f != "-shared"]
    tmp = tempfile.mkdtemp(prefix="adsb_dev_")
    try:
        objs = [os.path.join(tmp, "unit.o"), os.path.join(tmp, "driver.o")]
        cmds = [[B.hipcc()] + compile_flags + ["-c", src, "-o", objs[0]],
                [B.hipcc()] + compile_flags + ["-Wall", "-Wextra", "-c", drv, "-o", objs[1]]]
        jobs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in cmds]
        for c, p in zip(cmds, jobs):
            text = p.communicate()[0]
            assert p.returncode == 0, (c, text)
            assert "warning" not in text, (c, text)
        subprocess.check_call([B.hipcc()] + B.FLAGS + objs + ["-o", so])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print("built %s in %.1f s" % (os.path.relpath(so, HERE), time.time() - t0))
    return so
