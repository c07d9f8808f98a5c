"""CPU: the C-ABI shared library loads and exports every symbol include/txe.h declares (no compute calls without a
GPU), and the ctypes prototype table mirrors the header."""
import ctypes
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_decls():
    text = open(os.path.join(REPO, "include", "txe.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|size_t|float|unsigned)\s+(txe_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = [a.strip() for a in m.group(3).replace("\n", " ").split(",") if a.strip() and a.strip() != "void"]
        decls[m.group(2)] = (m.group(1), args)
    return decls


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "txe.h")).read(), flags=re.S)


def _header_structs():
    """every `struct txe_* { ... };` of the header as an ordered list of (field, C type or "*" for a pointer)"""
    structs = {}
    for m in re.finditer(r"\bstruct\s+(txe_\w+)\s*\{(.*?)\}\s*;", _header_text(), flags=re.S):
        fields = []
        for stmt in (x.strip() for x in m.group(2).replace("\n", " ").split(";")):
            if not stmt:
                continue
            first, *more = [d.strip() for d in stmt.split(",")]
            ctype, name = re.match(r"(.*?)(\w+)$", first).groups()          # `const float *` + `W`, `int ` + `n_nodes`
            base = ctype.replace("*", "").replace("const ", "").strip()
            fields.append((name, "*" if "*" in ctype else base))
            fields += [(d.lstrip("* "), "*" if d.startswith("*") else base) for d in more]      # `, *attn_l` / `, Kh`
        structs[m.group(1)] = fields
    return structs


def _header_constants():
    """every `NAME = value` of the header's enums and every `#define NAME value` with an integer value"""
    text = _header_text()
    vals = {k: int(v) for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, flags=re.S) for k, v in re.findall(r"(TXE_\w+)\s*=\s*(-?\d+)", body)}
    vals.update({k: int(v) for k, v in re.findall(r"#define\s+(TXE_\w+)\s+(-?\d+)\s*$", text, flags=re.M)})
    return vals


CMAP = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
        "unsigned long long": ctypes.c_ulonglong, "unsigned": ctypes.c_uint, "double": ctypes.c_double, "*": ctypes.c_void_p}


def test_ctypes_structures_mirror_the_header_structs():
    """every ctypes.Structure of _lib.py names a struct of include/txe.h in its docstring and has that struct's fields: same names, same
    order, same C types (pointers as c_void_p) -- and every struct of the header has such a mirror"""
    from taxoexpan_amd import _lib
    structs = _header_structs()
    mirrors = {}
    for obj in vars(_lib).values():
        if isinstance(obj, type) and issubclass(obj, ctypes.Structure) and obj is not ctypes.Structure:
            mirrors[re.match(r"struct (txe_\w+)", obj.__doc__).group(1)] = obj
    assert set(mirrors) == set(structs) and len(structs) >= 13, set(mirrors) ^ set(structs)
    for name, fields in structs.items():
        assert [(f, CMAP[t]) for f, t in fields] == [(f, t) for f, t in mirrors[name]._fields_], name
    # (the parser itself: a pointer list, a scalar list and a two-word type)
    gat = dict(structs["txe_gat_fold_layer"])
    assert gat["attn_l"] == "*" and gat["Pd"] == "int" and gat["seed"] == "unsigned long long" and gat["gid"] == "*" and gat["ld_hg"] == "long long"
    assert [f for f, _ in structs["txe_graph_batch"]] == ["rowptr_in", "col_src", "rowptr_out", "col_dst", "pos_out", "graph_off", "n_nodes", "n_edges", "G"]


def test_phase_and_flag_names_match_the_header():
    """the TXE_DENSE_* / TXE_FUSED_* / TXE_PH_* / TXE_FOLD_* bits of include/txe.h = the constants of the same names in _lib.py"""
    from taxoexpan_amd import _lib
    hdr = _header_constants()
    names = [k for k in hdr if k.startswith(("TXE_DENSE_", "TXE_FUSED_", "TXE_PH_", "TXE_FOLD_"))]
    assert len(names) == 17, names
    for k in names:
        assert getattr(_lib, k[4:]) == hdr[k], k
    mine = [k for k in vars(_lib) if k.startswith(("DENSE_", "FUSED_", "PH_", "FOLD_"))]
    assert sorted("TXE_" + k for k in mine) == sorted(names)
    assert hdr["TXE_FUSED_ALL"] == hdr["TXE_FUSED_DZ"] | hdr["TXE_FUSED_DW"] | hdr["TXE_FUSED_SWEEP"] | hdr["TXE_FUSED_REDUCE"]
    assert hdr["TXE_DENSE_ALL"] == hdr["TXE_DENSE_DX"] | hdr["TXE_DENSE_DW"] | hdr["TXE_DENSE_REDUCE"]
    assert hdr["TXE_TAIL_CHAIN_BYTES"] == _lib.TAIL_CHAIN_BYTES and hdr["TXE_ERR_ARG"] == -1


def test_library_builds_loads_and_exports_header_symbols():
    import __graft_entry__ as ge
    lib_path = ge.build()
    lib = ctypes.CDLL(lib_path)
    decls = _header_decls()
    assert len(decls) >= 26
    for name in decls:
        assert hasattr(lib, name), f"{name} declared in include/txe.h but not exported by libtxe.so"


def test_ctypes_table_mirrors_header():
    from taxoexpan_amd import _lib
    decls = _header_decls()
    assert set(decls) == set(_lib.SIGNATURES), set(decls) ^ set(_lib.SIGNATURES)
    cmap = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
            "unsigned long long": ctypes.c_ulonglong, "unsigned": ctypes.c_uint, "double": ctypes.c_double}
    for name, (ret, args) in decls.items():
        res, argtypes = _lib.SIGNATURES[name]
        assert res is cmap[ret], name
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is ctypes.c_void_p, (name, a)
            else:
                ctype = a.rsplit(" ", 1)[0].replace("const ", "").strip()
                assert t is cmap[ctype], (name, a, t)


def test_tail_chain_size_matches_the_header():
    """TXE_TAIL_CHAIN_BYTES (include/txe.h) = the buffer ops._TailChain hands to the C entry points"""
    import re
    from taxoexpan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "txe.h")).read()
    assert int(re.search(r"#define TXE_TAIL_CHAIN_BYTES (\d+)", hdr).group(1)) == _lib.TAIL_CHAIN_BYTES
    lib = _lib.load()
    assert lib.txe_gat_tail_flush(None, None) == 0                    # no chain: nothing to launch


def test_argument_validation_needs_no_gpu():
    """error paths return codes before anything is launched"""
    from taxoexpan_amd import _lib
    lib = _lib.load()
    assert lib.txe_gat_aggregate_fwd(None, None, 5, None, 0, None, None, 0, 4, 8, 0.2, 0.0, 0, 0, 1.0, None, 0, None, None, 0, None, 0.0, None,
                                     0, None) == -1
    assert lib.txe_readout_fwd(None, 3, None, 0, None, None, 8, None, None, None) == -1
    assert lib.txe_gat_dense_ws_bytes(100, 250, 50, 4, 500, 3) > 0
    assert lib.txe_gat_padded_k(250, 50) == 320 and lib.txe_gat_padded_f(4, 500) == 2048
    assert lib.txe_gat_aggregate_table_supported(4, 500, 2048, 3, 2080) == 1 and lib.txe_gat_aggregate_table_supported(5, 500, 2560, 3, 0) == 0
    assert lib.txe_gat_aggregate_table_fwd(None, None, 5, None, 2048, None, None, None, 3, 4, 500, 0.2, 0, 1.0, None, 0, None, 0, None, 0, None) == -1
    # the folded layers' entry points: a NULL descriptor, then descriptors whose required pointers are NULL
    ref = ctypes.addressof
    batch, gat, gcn = _lib.GraphBatch(n_nodes=5, n_edges=8, G=2), _lib.GatFoldLayer(Kh=16, Pd=4, D=8), _lib.GcnFoldLayer(Kh=16, Pd=4, Fo=8)
    below, grads, ggrads = _lib.GatFoldBelow(Hp=4, Dp=4), _lib.GatFoldGrads(), _lib.GcnFoldGrads()
    b, g, c, lo, gr, cg = (ref(x) for x in (batch, gat, gcn, below, grads, ggrads))
    for bb, ll in ((None, g), (b, None), (b, g)):
        assert lib.txe_gat_collapse_fwd(bb, ll, None, 0, None, 0, None) == -1
        assert lib.txe_gat_collapse_bwd(bb, ll, None, 8, 0, 1.0, None, gr, None, 0, None) == -1
        assert lib.txe_gat_collapse_bwd_fused(bb, ll, lo, None, gr, None, 8, 1.0, _lib.FUSED_ALL, None, 0, None, None, None, 0, None) == -1
    for bb, ll in ((None, c), (b, None), (b, c)):
        assert lib.txe_gcn_collapse_fwd(bb, ll, None, 0, None) == -1
        assert lib.txe_gcn_collapse_bwd(bb, ll, None, 8, 0, 1.0, None, cg, 0, None, 0, None) == -1
    assert lib.txe_gat_collapse_bwd(b, g, None, 8, 0, 1.0, None, None, None, 0, None) == -1
    assert lib.txe_gcn_collapse_bwd(b, c, None, 8, 0, 1.0, None, None, 0, None, 0, None) == -1
    for lo_, gr_ in ((None, gr), (lo, None)):
        assert lib.txe_gat_collapse_bwd_fused(b, g, lo_, None, gr_, None, 8, 1.0, _lib.FUSED_ALL, None, 0, None, None, None, 0, None) == -1
    # ... and with every pointer in place (never read: host memory, and no workspace) the checks run in the old order: the fused
    # backward refuses a (Kh, Pd, Hp, Dp) it does not support before it looks at the workspace, which is what all five refuse last
    buf = (ctypes.c_float * 64)()
    a = ref(buf)
    batch = _lib.GraphBatch(a, a, a, a, a, a, 5, 8, 2)
    gat = _lib.GatFoldLayer(X=a, Kh=16, Pd=4, pos=a, vocab=3, Wp=a, W=a, attn_l=a, attn_r=a, D=8, a12=a, alpha=a, coef=a, wsum=a, gid=a, Z=a, hg=a, ld_hg=8)
    gcn = _lib.GcnFoldLayer(X=a, Kh=16, Pd=4, pos=a, vocab=3, Wp=a, Fo=8, norm=a, coef=a, wsum=a, gid=a, Z=a, hg=a, ld_hg=8)
    grads, ggrads = _lib.GatFoldGrads(a, a, a, a, a), _lib.GcnFoldGrads(a, a, a, a)
    b, g, c, gr, cg = (ref(x) for x in (batch, gat, gcn, grads, ggrads))
    for Hp, Dp, want in ((3, 4, -1), (4, 8, -1), (4, 3, -1), (4, 4, -3)):     # 3 heads; Hp * Dp != Kh; Dp no multiple of 4; supported
        assert lib.txe_gat_fused_bwd_supported(16, 4, Hp, Dp) == (want == -3)
        below = _lib.GatFoldBelow(Yp=a, ld_yp=128, Hp=Hp, Dp=Dp, alpha_p=a, d_Yp=a, ld_dyp=128, n_pad=0, dz_p=a)
        assert lib.txe_gat_collapse_bwd_fused(b, g, ref(below), None, gr, a, 8, 1.0, _lib.FUSED_ALL, None, 0, None, None, a, 0, None) == want
    assert lib.txe_gat_collapse_fwd(b, g, None, 0, a, 0, None) == -3
    assert lib.txe_gat_collapse_bwd(b, g, a, 8, 0, 1.0, a, gr, a, 0, None) == -3
    assert lib.txe_gcn_collapse_fwd(b, c, a, 0, None) == -3
    assert lib.txe_gcn_collapse_bwd(b, c, a, 8, 0, 1.0, a, cg, 0, a, 0, None) == -3
    gat.feat_drop_p = gcn.drop_p = 1.0                                       # (a scalar out of range, read through the descriptor)
    assert lib.txe_gat_collapse_fwd(b, g, None, 0, a, 0, None) == -1 and lib.txe_gcn_collapse_fwd(b, c, a, 0, None) == -1

def test_host_rng_restatement_matches_library():
    """taxoexpan_amd/rng.py == the hash the kernels inline (evaluated on the host by the library)"""
    from taxoexpan_amd import _lib, rng
    lib = _lib.load()
    for seed in (0, 1, 123456789, 2 ** 61 + 12345):
        idx = np.array([0, 1, 2, 63, 64, 1000, 2 ** 31, 2 ** 40 + 17], dtype=np.uint64)
        want = np.array([lib.txe_dropout_uniform_host(seed, int(i)) for i in idx], dtype=np.float32)
        got = rng.uniform01(seed, idx)
        assert np.array_equal(got, want)
    m = rng.keep_mask(42, (1000, 37), 0.3)
    assert abs(m.mean() - 0.7) < 0.01
    # bit-mask form used for feature dropout: words from the library (host evaluation) == rng.keep_mask_bits
    for seed, rows, cols, p in ((7, 5, 70, 0.1), (2 ** 40 + 3, 3, 32, 0.3), (11, 4, 17, 0.5)):
        wpr = (cols + 31) // 32
        bits = rng.keep_mask_bits(seed, rows, cols, p)
        for r in range(rows):
            for w in range(wpr):
                word = lib.txe_dropout_mask_word_host(seed, r * wpr + w, p)
                for b in range(32):
                    c = w * 32 + b
                    if c < cols:
                        assert bits[r, c] == ((word >> b) & 1), (seed, r, c)
    assert abs(rng.keep_mask_bits(5, 500, 300, 0.1).mean() - 0.9) < 0.005


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from taxoexpan_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    try:
        _lib.call("txe_gcn_norm", None, 0, None, None)
    except _lib.TxeError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("expected TxeError")


def test_ops_refuse_host_tensors():
    import pytest
    import torch
    from taxoexpan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bilinear_project(torch.zeros(4, 3), torch.zeros(1, 3, 2))


def test_lds_direct_copies_are_the_only_users_of_m0():
    """csrc/txe_gemm_split.hip issues its global -> LDS copies from inline asm (`s_mov_b32 m0, <lds address>` + `global_load_lds_dwordx4`):
    M0 is a reserved register that cannot be named in a clobber list, so the source cannot tell the compiler about it.  What CAN be
    checked is the generated gfx950 ISA: in that file every mention of m0 is such a move, immediately followed by the copy that reads
    it -- no compiler-generated M0 user (readlane/movrel, s_sendmsg, GWS, LDS-direct ds_* with M0) exists for the asm to corrupt."""
    import re
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(REPO, "taxoexpan_amd", "csrc", "txe_gemm_split.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "split.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", out],
                           capture_output=True, text=True, cwd=os.path.dirname(src))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln.strip() for ln in open(out) if ln.strip() and not ln.strip().startswith((";", ".", "//"))]
    uses = [i for i, ln in enumerate(lines) if re.search(r"\bm0\b", ln.split(";")[0])]
    assert len(uses) >= 20                                   # the copies are there
    for i in uses:
        assert re.match(r"s_mov_b32 m0, s\d+", lines[i]), lines[i]
        assert lines[i + 1].startswith("global_load_lds_dwordx4"), (lines[i], lines[i + 1])
