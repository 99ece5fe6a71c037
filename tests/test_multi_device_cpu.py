"""Device list of the host-level entry points (svt_set_devices, include/svt_hip.h) without a GPU: the symbols,
the loud failure on a box without an MI355X, and the R glue's reading of SPARSEARRAY_HIP_DEVICES
(integration/svt_hip_glue.c, hip_available()) against a recording stand-in for the library."""
import ctypes
import os
import subprocess
import sys
import textwrap

import pytest

import glue_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_list_symbols_are_exported():
    from sparsearray_amd._hip import EXPORTS, load_library
    lib = load_library()
    for sym in ("svt_set_devices", "svt_get_devices", "svt_set_shard_min_nnz"):
        assert sym in EXPORTS
        assert hasattr(lib, sym), sym


def test_set_devices_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sparsearray_amd._hip import load_library
    lib = load_library()
    arr = (ctypes.c_int * 2)(0, 0)
    assert lib.svt_set_devices(arr, 2) == -1
    assert b"no HIP device" in lib.svt_last_error()
    assert lib.svt_get_devices(arr, 2) == 0          # no list was set
    lib.svt_set_shard_min_nnz(0)                     # (no device needed)


_RECORDER = r"""
#include <stdio.h>
#include <string.h>
static int g_calls = -1, g_list[32];
int svt_init(int device) { (void) device; return 0; }
const char *svt_last_error(void) { return ""; }
int svt_set_max_threads(int n) { return n; }
int svt_set_devices(const int *o, int n) { g_calls = n; for (int i = 0; i < n && i < 32; i++) g_list[i] = o[i]; return 0; }
int rec_calls(void) { return g_calls; }
int rec_dev(int i) { return g_list[i]; }
"""

_DRIVER = r"""
import ctypes, os, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import glue_harness
g = glue_harness.Glue({harness!r}, {shim!r})
g.call("C_set_max_threads", g.ints(2))
rec = ctypes.CDLL({shim!r})
n = rec.rec_calls()
print(",".join(str(rec.rec_dev(i)) for i in range(n)) if n >= 0 else "none")
"""


@pytest.fixture(scope="module")
def glue_build(tmp_path_factory):
    why = glue_harness.ref_build_unavailable()
    if why is not None:
        pytest.skip(why)
    d = str(tmp_path_factory.mktemp("glue_devices"))
    harness, _ = glue_harness.build(d)
    src = os.path.join(d, "recorder.c")
    with open(src, "w") as f:
        f.write(_RECORDER)
    shim = os.path.join(d, "librecorder.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-Wall", src, "-o", shim])
    return harness, shim


def _glue_devices(glue_build, value):
    harness, shim = glue_build
    env = dict(os.environ)
    env.pop("SPARSEARRAY_HIP_DEVICES", None)
    if value is not None:
        env["SPARSEARRAY_HIP_DEVICES"] = value
    code = textwrap.dedent(_DRIVER.format(tests=os.path.join(ROOT, "tests"), root=ROOT, harness=harness, shim=shim))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("value,want", [
    ("0,1,2,3", "0,1,2,3"),
    ("0,0,0,0", "0,0,0,0"),
    ("3", "3"),
    (" 1 , 2 ", "1,2"),
    (",".join(["0"] * 16), ",".join(["0"] * 16)),
])
def test_glue_passes_the_device_list(glue_build, value, want):
    assert _glue_devices(glue_build, value) == want


@pytest.mark.parametrize("value", [None, "", "a", "0,", ",0", "0,,1", "-1", "0;1", "1.5", ",".join(["0"] * 17)])
def test_glue_keeps_one_device_on_absent_or_malformed_lists(glue_build, value):
    assert _glue_devices(glue_build, value) == "none"
