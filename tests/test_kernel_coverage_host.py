"""Every kernel-level entry point of include/qst_kernels.h is called by name from some GPU test.

A kernel that is reached only through a whole-encoder run, or only through a dispatcher that picks it by shape or by a mode
switch, is checked at the preset shapes and the loose tolerances of an end-to-end comparison, if at all. This test keeps
that gap from reopening as entry points are added: a name counts as covered when a tests/test_gpu_*.py file calls it as
`lib.NAME`, or names its base in `kf(lib, "NAME", op)` / `_lib.kfn(lib, "NAME", op)`, which covers the `_f16` twin too.
"""
import fnmatch
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qst_kernels.h")
TESTS = os.path.join(ROOT, "tests")

# Entry points that launch nothing: capability and size queries, and process-wide mode switches. The kernels they describe
# or steer are called by name elsewhere.
ALLOW = [
    "*_supported", "*_supported_f16",        # shape / epilogue queries
    "*_block_rows*",                         # rows per partial-sum block of the fused GEMM + LayerNorm
    "*_bytes",                               # scratch sizes
    "*_timeouts*",                           # sticky host-side read of the exchange's timeout word
    "qst_gemm8_stagger",                     # mode switches (return the previous value)
    "qst_gemm8_ln_store",
    "qst_gemm8_mode",
    "qst_abi_sizeof",                        # struct sizes for the ctypes mirror (tests/test_abi_layout.py)
]

_DECL = re.compile(r"^(?:int|int64_t|size_t|void)\s+\**\s*(qst_\w+)\s*\(", re.M)


def declared():
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)       # block comments (examples in them are not declarations)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(_DECL.findall(text)))


def called():
    direct, bases = set(), set()
    for fn in sorted(os.listdir(TESTS)):
        if not (fn.startswith("test_gpu_") and fn.endswith(".py")):
            continue
        with open(os.path.join(TESTS, fn)) as f:
            src = f.read()
        direct.update(re.findall(r"\blib\.(qst_\w+)", src))
        bases.update(re.findall(r"\bkfn?\(\s*lib\s*,\s*[\"'](qst_\w+)[\"']", src))
    return direct, bases


def uncovered(names, direct, bases):
    out = []
    for n in names:
        if any(fnmatch.fnmatchcase(n, p) for p in ALLOW):
            continue
        base = n[:-4] if n.endswith("_f16") else n
        if n in direct or n in bases or base in bases:
            continue
        out.append(n)
    return out


def test_header_parse_finds_the_entry_points():
    names = declared()
    # a parser that silently matched nothing would make the coverage check below vacuous
    assert len(names) >= 90
    for n in ("qst_gemm_nt", "qst_embed_ln_fwd_f16", "qst_shadow_all_split_f16", "qst_ln_bwd_reduce_batch",
              "qst_dropout_apply_f32", "qst_abi_sizeof"):
        assert n in names


def test_every_entry_point_is_called_by_name_from_a_gpu_test():
    direct, bases = called()
    missing = uncovered(declared(), direct, bases)
    assert not missing, ("entry points of include/qst_kernels.h that no tests/test_gpu_*.py calls by name "
                         f"(lib.NAME or kf(lib, \"NAME\", op)): {missing}")


def test_allowlist_names_only_entry_points_that_exist():
    names = declared()
    for p in ALLOW:
        assert any(fnmatch.fnmatchcase(n, p) for n in names), f"allowlist entry {p!r} matches no declaration"


def test_kf_base_name_covers_the_f16_twin_only():
    assert uncovered(["qst_x", "qst_x_f16"], set(), {"qst_x"}) == []
    assert uncovered(["qst_x", "qst_x_f16"], {"qst_x"}, set()) == ["qst_x_f16"]
    assert uncovered(["qst_y_supported"], set(), set()) == []
