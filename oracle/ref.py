"""TEST INFRASTRUCTURE ONLY -- oracle/_ref/: what the glue tests take from the reference.

`make -C oracle ref REF=<tree>` (oracle/Makefile) compiles it from a SparseArray source tree; build() runs it,
and tests/glue_harness.py runs it again when oracle/_ref/ is missing or was compiled from other files of this
repository.  Nothing of the reference is kept in the repository.
"""
from __future__ import annotations

import os
import pwd
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_BUILD = os.path.join(HERE, "_ref")
NAMES = ("reference", "SparseArray")


def _is_tree(path: str) -> bool:
    try:
        with open(os.path.join(path, "DESCRIPTION")) as f:
            if "Package: SparseArray" not in f.read():
                return False
    except OSError:
        return False
    return os.access(os.path.join(path, "src", "argcheck_utils.c"), os.R_OK)


def reference_tree() -> str | None:
    """A readable SparseArray source tree: $SPARSEARRAY_SRC, else a directory named `reference` or `SparseArray`
    beside this repository or beside one of its parent directories, or in the home directory of this user or of
    any user of the host; None when there is none."""
    cands = [os.environ.get("SPARSEARRAY_SRC")]
    d = ROOT
    while True:
        up = os.path.dirname(d)
        cands += [os.path.join(up, n) for n in NAMES]
        if up == d:
            break
        d = up
    homes = [os.path.expanduser("~")]
    try:
        homes += sorted({p.pw_dir for p in pwd.getpwall() if p.pw_dir})
    except OSError:
        pass
    cands += [os.path.join(h, n) for h in homes for n in NAMES]
    for c in cands:
        if c and _is_tree(c):
            return os.path.abspath(c)
    return None


def build_ref(ref: str | None = None) -> tuple[bool, str]:
    """Runs the `ref` recipe; (False, why) when there is no tree or make fails."""
    ref = ref or reference_tree()
    if ref is None:
        return False, "no SparseArray source tree found (SPARSEARRAY_SRC)"
    p = subprocess.run(["make", "-s", "-C", HERE, "ref", f"REF={ref}"], capture_output=True, text=True)
    return p.returncode == 0, p.stdout + p.stderr
