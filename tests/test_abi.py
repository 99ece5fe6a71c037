"""The C-ABI library loads and exports every symbol include/svt_hip.h declares
(no compute calls: runs without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(svt_[A-Za-z0-9_]+)\s*\(", text)))


def _ctype(decl, what):
    """One parameter or return type of the header, by the mapping rule of sparsearray_amd/_abi.py; an unknown one fails."""
    import ctypes
    from sparsearray_amd._abi import ALLOC_FN, FREE_FN
    scalars = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "double": ctypes.c_double,
               "svt_dev_alloc_fn": ALLOC_FN, "svt_dev_free_fn": FREE_FN}
    words = re.sub(r"\bconst\b", " ", decl).split()
    if "*" in decl or "[" in decl:
        if what == "return":
            return ctypes.c_char_p if words == ["char", "*"] else ctypes.c_void_p
        return ctypes.c_void_p
    if what == "return" and words == ["void"]:
        return None
    base = words[0] if 1 <= len(words) <= (1 if what == "return" else 2) else None        # "type" or "type name"
    assert base in scalars, f"{what} {decl!r}: a type the mapping rule does not know"
    return scalars[base]


def _header_prototypes():
    """{name: (restype, [argtypes])} of every function include/svt_hip.h declares.  A statement that is neither a
    typedef, an enum nor `ret svt_name(args)` fails."""
    text = open(os.path.join(ROOT, "include", "svt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M).replace('extern "C" {', " ")
    text = re.sub(r"\{[^{}]*\}", " ", text)                                   # struct and enum bodies
    protos = {}
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if not stmt or stmt == "}" or stmt.startswith(("typedef ", "enum")):
            continue
        m = re.fullmatch(r"(.+?)\b(svt_\w+) ?\((.*)\)", stmt)
        assert m, f"not a function declaration: {stmt!r}"
        ret, name, args = m.groups()
        assert name not in protos, name
        protos[name] = (_ctype(ret.replace("*", " * "), "return"),
                        [] if args.strip() == "void" else [_ctype(a, "parameter") for a in args.split(",")])
    return protos


def test_prototype_table_matches_the_header():
    """sparsearray_amd/_abi.py states the header's prototypes: the same names, and per name the same return type,
    arity and per-argument type.  (A Python int passed without a prototype goes as a 32-bit int: a missing or wrong
    row truncates a device pointer, an int64_t count or a size_t.)"""
    from sparsearray_amd._abi import PROTOTYPES
    want = _header_prototypes()
    assert sorted(want) == _declared_symbols()                # the parser saw every declaration
    assert sorted(PROTOTYPES) == sorted(want)
    for name, (restype, argtypes) in want.items():
        got_res, got_args = PROTOTYPES[name]
        assert got_res is restype, f"{name}: returns {restype}, the table says {got_res}"
        assert len(got_args) == len(argtypes), f"{name}: {len(argtypes)} parameters, the table has {len(got_args)}"
        for k, (g, w) in enumerate(zip(got_args, argtypes)):
            assert g is w, f"{name}: parameter {k} is {w}, the table says {g}"


def test_load_applies_the_whole_table():
    from sparsearray_amd._abi import PROTOTYPES
    from sparsearray_amd._hip import load_library
    lib = load_library()
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


def test_dispatcher_declares_by_prefix():
    """CAbiDispatcher sets the table's prototype on <prefix><name> for the names its library has, and on nothing else."""
    import types
    from sparsearray_amd._abi import PROTOTYPES
    from sparsearray_amd._dispatch import CAbiDispatcher
    names = ["last_error", "colStats_SVT", "crossprod2_SVT_mat", "transpose_2D_SVT", "get_num_procs"]
    stub = types.SimpleNamespace(**{"chk_" + n: types.SimpleNamespace() for n in names},
                                 chk_dotprod_ints_zero=types.SimpleNamespace(),          # no row of the table
                                 svt_rowsum_SVT=types.SimpleNamespace())                 # another prefix
    CAbiDispatcher(stub, "chk_")
    for n in names:
        f = getattr(stub, "chk_" + n)
        assert (f.restype, f.argtypes) == PROTOTYPES["svt_" + n], n
    assert vars(stub.chk_dotprod_ints_zero) == {} and vars(stub.svt_rowsum_SVT) == {}
    assert sorted(vars(stub)) == sorted(["chk_" + n for n in names] + ["chk_dotprod_ints_zero", "svt_rowsum_SVT"])


def test_header_and_export_list_agree():
    from sparsearray_amd._hip import EXPORTS
    assert sorted(EXPORTS) == _declared_symbols()


def test_library_exports_every_declared_symbol():
    from sparsearray_amd._hip import load_library
    lib = load_library()
    for sym in _declared_symbols():
        assert hasattr(lib, sym), f"libsvt_hip.so does not export {sym}"


def test_thread_control_entry_points_need_no_gpu():
    """C_get_num_procs / C_get_max_threads / C_set_max_threads (src/thread_control.c:47-66):
    set returns the previous value, get returns what was set."""
    from sparsearray_amd._hip import load_library
    lib = load_library()
    assert lib.svt_get_num_procs() >= 1
    first = lib.svt_get_max_threads()
    assert first >= 1
    assert lib.svt_set_max_threads(3) == first
    assert lib.svt_get_max_threads() == 3
    assert lib.svt_set_max_threads(first) == 3


def test_product_fails_loudly_without_gpu():
    """On a box without an MI355X the product path must raise, not fall back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sparsearray_amd
    from sparsearray_amd._hip import HipBackendError
    with pytest.raises(HipBackendError, match="no HIP device|gfx950"):
        sparsearray_amd.hip_session()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "sparsearray_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                for needle in ("import oracle", "from oracle", "svt_oracle", "orc_"):
                    assert needle not in src, f"{f} references the oracle ({needle})"


def test_generated_asm_is_in_sync(tmp_path):
    """sparsearray_amd/csrc/pbc_dma_asm.inc is generated (tools/gen_pbc_asm.py) and committed:
    the committed text must be what the generator writes with its defaults."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "pbc_dma_asm.inc"
    env = {k: v for k, v in os.environ.items() if not k.startswith("PBC_")}
    env["PBC_ASM_OUT"] = str(out)
    subprocess.run([sys.executable, os.path.join(root, "tools", "gen_pbc_asm.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    committed = open(os.path.join(root, "sparsearray_amd", "csrc", "pbc_dma_asm.inc")).read()
    assert out.read_text() == committed


def test_generated_gatherx_asm_is_in_sync(tmp_path):
    """sparsearray_amd/csrc/pbgx_asm.inc (the pass loop of the XCD-paced gather kernel) is what
    tools/gen_pbgx_asm.py writes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "pbgx_asm.inc"
    env = dict(os.environ)
    env["PBGX_ASM_OUT"] = str(out)
    subprocess.run([sys.executable, os.path.join(root, "tools", "gen_pbgx_asm.py")], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    committed = open(os.path.join(root, "sparsearray_amd", "csrc", "pbgx_asm.inc")).read()
    assert out.read_text() == committed
