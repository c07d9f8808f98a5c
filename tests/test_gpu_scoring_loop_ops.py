"""The all-candidate scoring and ranking loop (the second half of csrc/txe_match.hip, csrc/txe_rank.hip, the pick / count / best-k modes of
gemm_tile_epilogue, the EPI == 2 instance of gemm_nt_split_kernel) against an INDEPENDENT reference, entry point by entry point, through
the C ABI: the test owns every pitch, pointer offset, scratch buffer and workspace.

Reference: tests/scoring_loop_ref.py (plain numpy, float64 and integers; tests/test_scoring_loop_ref_cpu.py holds it to the project's host
code and the goldens, and its case tables to the branches they are there for).
  (a) score VALUES, generic inputs: txe_score_block and txe_score_positives against float64 through golden_util.gate_against_f64 at its
      defaults (yardstick: the numpy fp32 product + fp32 exp), both apply_exp values, three routes: the fp32 MFMA (sws NULL), the bf16
      pipe packing per call, the bf16 pipe with u_packed from txe_split_pack.  Every gate prints "[gate] op what device yardstick".
      One exp case plants raw scores of 95, 89.5, -106, -110: inf / 0 in fp32, compared on the pattern and kept out of the gate.
  (b) INTEGER results, exact inputs (multiples of 1/4: every fp32 sum is exact in any order, on either pipe), no tolerance: scores
      bit-equal to float64 cast to fp32 (under the exp: equal raw scores give equal bits, distinct ones keep their order); counts for
      thresholds the test supplies (the positive's own score, that + 1/8, -inf, +inf, NaN) and for those txe_score_positives wrote;
      txe_rank_finalize of them == the metric's definition; best k for k = 1, 5, 8 with idx_base 7.  The NaN / Inf variant goes through
      all four entry points on all three routes (on the bf16 pipe: the fp32 recompute of a tile under the pick, count and best-k epilogues).
  (c) txe_rank_block, txe_rank_finalize, txe_topk_merge alone on arrays the test writes: heavy ties, NaN, +-inf, -0.0 beside +0.0, real
      -inf keys beside empty slots, NaN keys.

NaN priming: S lies inside its pitch padding with a guard row before and behind it -- all still NaN afterwards; thr has a NaN tail; counts
are primed with 1000 + j and come back as that PLUS the reference (the header's +=); every scratch buffer (part_key, part_idx, floor_ws,
sws, the tail workspace, the packed planes) starts as NaN / 0x7fc00000, and the words behind its documented size keep that.  Every call
asserts the launch names its profiler recorded against scoring_loop_ref.launches at the DEVICE's CU count (rank_kernel,
rank_finalize_kernel and topk_floor_init_kernel record nothing: their results, and floor_ws, are what is asserted).  A rejected call
returns its code, records no launch and leaves outputs and scratch primed.

Instance -> case:
    gemm_kernel<true, true, {4/4, 4/2, 2/4, 2/2, 1/1}, 64> plain / pick / count, <..., 128> best-k       test_exact_integer_results (sl.SCORE_CASES)
    gemm_kernel<true, true, 4, 4, 128> plain / pick / count (sized by the CU count)                     test_exact_integer_results[wide]
    gemm_nt_split_kernel<2, 3, 2, 2> under all four epilogues, packed per call and with u_packed         the same cases, routes "split" / "packed"
    count epilogue past PS = 8 thresholds (E.cnt_thr[pb + k]): 9, 17, 300 positives                     127x3x10 .. 300x1003x32, wide
    gemm_persist_kernel<true, true, 4, 4>, whole rounds / leftover whole tiles                          test_persistent_score_kernel
    rank_kernel 16-byte and scalar paths, rank_finalize_kernel, topk_merge_kernel                       test_rank_block_alone, test_topk_merge_alone
(The best-k epilogue has no 64-wide instance: force_bn128.  rank_kernel's second g0 round starts at 1,025 chunks, G = 4,101: the table
holds 4,097 -- one full round and a ragged end -- and 4,101.)

What the tests found, fixed in the same change: txe_score_topk_block initialised floor_ws (a launch) before it rejected a short sws;
none of the four score entry points checked ld_q >= r, txe_score_block not ld_s >= G; txe_topk_merge left out_key unwritten at cnt == 0
and dropped entries whose key is NaN (now -inf in out_key's unused slots, as txe_select_k; a NaN key counts as -inf: it ranks last).

Measured on the MI355X (256 CUs), one run of the file: 59 cases (70 gated tensors) in 7.5 s, the slowest test_exact_integer_results[wide-exp]
(512 x 8,201, three routes) 2.3 s, test_persistent_score_kernel (two 1,024 x 16,6xx x 160 blocks) 0.2 s; tests/test_scoring_loop_ref_cpu.py:
29 cases in 6 s on the CPU.  Errors as fractions of the tensor's largest float64 entry; largest device / yardstick ratio, largest device error:
    txe_score_block, fp32 MFMA        1.15 (300 x 1003 x 32, no exp: 2.2e-7 against 2.0e-7); largest 8.4e-7
    txe_score_block, bf16 pipe        1.00 on both forms; largest 5.4e-7
    txe_score_positives, fp32 MFMA    1.30 (no exp: 5.8e-8 against 4.5e-8); largest 8.7e-7
    txe_score_positives, bf16 pipe    1.00; largest 4.1e-7
Under the exp, largest per-entry RELATIVE error against float64 (generic inputs, r up to 250: the raw score's own rounding is in it):
device 1.8e-6 on the fp32 MFMA, 1.4e-6 on the bf16 pipe (both forms), the fp32 yardstick (fp32 product, fp32 exp) 1.8e-6 -- __expf costs
nothing that shows beside the product's rounding.  On exact raw scores all three routes give the same bits.
The mutation pass and the comparison with the parent commit: profiles/NOTES.md, "Scoring loop against float64".
"""
import numpy as np
import pytest
import torch

import scoring_loop_ref as sl
from golden_util import gate_against_f64
from test_gpu_readout_match_ops import _profiled

pytestmark = pytest.mark.gpu

NAN = float("nan")
NANI = 0x7FC00000
GUARD = 64
ROUTES = ("mfma", "split", "packed")


def _dev():
    return torch.device("cuda:0")


def _L():
    from taxoexpan_amd import _lib
    return _lib


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rc(name, *args):
    """the entry point's return code (no exception)"""
    return getattr(_L().load(), name)(*args)


def _ok(name, *args):
    rc = _rc(name, *args)
    assert rc == 0, (name, rc)
    return rc


def _st():
    return _L().stream_ptr()


def _nan(n):
    return torch.full((max(int(n), 1),), NAN, device=_dev())


def _nani(n):
    return torch.full((max(int(n), 1),), NANI, dtype=torch.int32, device=_dev())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _laid(a, ld, off):
    """a [rows][cols] on a pitch of ld floats, `off` floats behind an aligned allocation whose every other word is NaN: (buffer, pointer)"""
    rows, cols = a.shape
    buf = _nan(off + rows * ld + 4)
    assert buf.data_ptr() % 256 == 0
    if rows:
        buf[off:off + rows * ld].view(rows, ld)[:, :cols].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, buf.data_ptr() + 4 * off


def _tail_intact(t, n):
    """the words of a primed buffer from n on are untouched"""
    tail = t[n:]
    assert bool(torch.isnan(tail).all()) if t.dtype == torch.float32 else bool((tail == NANI).all()), "words behind the buffer's documented size were written"


def _gate(op, items):
    errors, report = [], []
    for what, got, ref64, yard in items:
        gate_against_f64(got, ref64, yard, what, errors, report=report)
    for what, e_dev, e_yard in report:
        print(f"[gate] {op} {what} {e_dev:.3e} {e_yard:.3e}")
    assert not errors, (op, errors, report)


# ---- one case's inputs on the host and the device -------------------------------------------------------------------------------------------
class _Inputs:
    def __init__(self, Q, U, pos_off, pos_idx, ld_q, off_q, ld_u, off_u, ld_s, off_s):
        self.Q, self.U, self.pos_off, self.pos_idx = Q, U, pos_off, pos_idx
        self.nq, self.r = Q.shape
        self.G = U.shape[0]
        self.n_pos = int(pos_off[-1])
        self.ld_q, self.off_q, self.ld_u, self.off_u, self.ld_s, self.off_s = ld_q, off_q, ld_u, off_u, ld_s, off_s
        self.Qb, self.Qp = _laid(Q, ld_q, off_q)
        self.Ub, self.Up_ = _laid(U, ld_u, off_u)
        self.Pb, self.Pp = _laid(U[pos_idx], ld_u, off_u)                   # the positives' candidate rows, query by query
        self.offd, self.idxd = _up(pos_off), _up(pos_idx if len(pos_idx) else np.zeros(1, dtype=np.int32))
        self._planes = None

    def names(self, entry, route, tail=False):
        N = self.n_pos if entry == "positives" else self.G
        if entry == "positives" and route == "packed":
            route = "split"                                                 # (txe_score_positives takes no u_packed: its rows change per block)
        return sl.launches(entry, route, self.nq, N, self.r, self.ld_q, self.off_q, self.ld_u, self.off_u, tail, _cus())

    def planes(self):
        """the candidates' planes, made once (txe_split_pack, side 1) into a NaN-primed buffer"""
        if self._planes is None:
            L = _L()
            nb = L.call("txe_split_packed_bytes", self.G, self.r)
            assert nb > 0 and nb % 4 == 0
            buf = _nan(nb // 4 + GUARD)
            _rc_, names = _profiled(lambda: _ok("txe_split_pack", self.Up_, self.ld_u, self.G, self.r, 1, buf.data_ptr(), _st()))
            assert names == ["split_pack_kernel"]
            _tail_intact(buf, nb // 4)
            self._planes = buf
        return self._planes

    def sws(self, route, entry):
        """(buffer, pointer, bytes, u_packed pointer) of a route"""
        if route == "mfma":
            return None, None, 0, None
        L = _L()
        N = self.n_pos if entry == "positives" else self.G
        if route == "packed" and entry != "positives":
            nb = sl.round_up(L.call("txe_split_packed_bytes", self.nq, self.r), 256)
            upk = self.planes().data_ptr()
        else:
            nb, upk = L.call("txe_score_split_ws_bytes", self.nq, N, self.r), None
        buf = _nan(nb // 4 + GUARD)
        return buf, buf.data_ptr(), nb, upk


def _score_block(I, route, exp, tail=False):
    """txe_score_block into S inside its pitch padding and guard rows: the [nq][G] scores; everything around them still NaN"""
    nq, G, ld = I.nq, I.G, I.ld_s
    buf = _nan(I.off_s + (nq + 2) * ld + 4)
    sp = buf.data_ptr() + 4 * (I.off_s + ld)
    sb, swp, swb, upk = I.sws(route, "block")
    ws, wsb = None, 0
    if tail:
        wsb = _L().call("txe_gemm_tail_ws_bytes")
        ws = _nan(wsb // 4 + GUARD)
    _r, names = _profiled(lambda: _ok("txe_score_block", I.Qp, I.ld_q, nq, I.Up_, I.ld_u, G, I.r, int(exp), sp, ld, _ptr(ws), wsb, swp, swb, upk, _st()))
    assert names == I.names("block", route, tail), (names, I.names("block", route, tail))
    a = buf.cpu().numpy()
    body = a[I.off_s + ld:I.off_s + (nq + 1) * ld].reshape(nq, ld)
    assert np.isnan(a[:I.off_s + ld]).all() and np.isnan(a[I.off_s + (nq + 1) * ld:]).all(), "a guard row of S was written"
    assert np.isnan(body[:, G:]).all(), "the pitch padding of S was written"
    if sb is not None:
        _tail_intact(sb, swb // 4)
    if ws is not None:
        _tail_intact(ws, wsb // 4)
    return body[:, :G].copy()


def _score_positives(I, route, exp):
    thr = _nan(I.n_pos + 8)
    sb, swp, swb, _upk = I.sws(route, "positives")
    _r, names = _profiled(lambda: _ok("txe_score_positives", I.Qp, I.ld_q, I.nq, I.Pp, I.ld_u, I.n_pos, I.r, int(exp), I.offd.data_ptr(), thr.data_ptr(), swp, swb, _st()))
    assert names == I.names("positives", route), (names, I.names("positives", route))
    _tail_intact(thr, I.n_pos)
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return thr.cpu().numpy()[:I.n_pos].copy()


def _count(I, route, exp, thr, larger):
    """txe_score_count_block on thresholds `thr` (fp32, any values): counts MINUS their priming"""
    n = I.n_pos
    prime = (1000 + np.arange(n + 8)).astype(np.int32)
    cd, td = _up(prime), _nan(n + 8)
    td[:n].copy_(torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)))
    sb, swp, swb, upk = I.sws(route, "count")
    _r, names = _profiled(lambda: _ok("txe_score_count_block", I.Qp, I.ld_q, I.nq, I.Up_, I.ld_u, I.G, I.r, int(exp), I.offd.data_ptr(), td.data_ptr(), int(larger),
                                       cd.data_ptr(), swp, swb, upk, _st()))
    assert names == I.names("count", route), (names, I.names("count", route))
    got = cd.cpu().numpy()
    assert np.array_equal(got[n:], prime[n:]), "counts behind the last positive were written"
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return (got[:n] - prime[:n]).astype(np.int64), td


def _finalize(I, td, cnt, larger):
    n = I.n_pos
    cd, rk = _up(cnt.astype(np.int32)) if n else _nani(1), _nani(n + 8)
    _r, names = _profiled(lambda: _ok("txe_rank_finalize", I.offd.data_ptr(), I.nq, td.data_ptr(), cd.data_ptr(), int(larger), rk.data_ptr(), _st()))
    assert names == []
    _tail_intact(rk, n)
    return rk.cpu().numpy()[:n].astype(np.int64)


def _topk(I, route, exp, larger, k, idx_base, with_key=True):
    nq, tiles = I.nq, _L().call("txe_score_topk_tiles", I.G)
    assert tiles == sl.topk_tiles(I.G)
    pk, pi, fl = _nan(nq * tiles * k + 8), _nani(nq * tiles * k + 8), _nani(nq + 8)
    oi, okey = _nani(nq * k + 8), (_nan(nq * k + 8) if with_key else None)
    sb, swp, swb, upk = I.sws(route, "topk")
    _r, names = _profiled(lambda: _ok("txe_score_topk_block", I.Qp, I.ld_q, nq, I.Up_, I.ld_u, I.G, I.r, int(exp), int(larger), k, idx_base, pk.data_ptr(), pi.data_ptr(),
                                       fl.data_ptr(), oi.data_ptr(), _ptr(okey), swp, swb, upk, _st()))
    assert names == I.names("topk", route), (names, I.names("topk", route))
    for t, n in ((pk, nq * tiles * k), (pi, nq * tiles * k), (fl, nq), (oi, nq * k)) + (((okey, nq * k),) if with_key else ()):
        _tail_intact(t, n)
    if sb is not None:
        _tail_intact(sb, swb // 4)
    return oi.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.int64), (okey.cpu().numpy()[:nq * k].reshape(nq, k) if with_key else None)


# ---- (a) values against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exp", [0, 1])
@pytest.mark.parametrize("case", range(len(sl.GENERIC_CASES)), ids=["x".join(map(str, c[:3])) for c in sl.GENERIC_CASES])
def test_score_values_against_float64(case, exp):
    """txe_score_block (with and without the tail workspace) and txe_score_positives on generic inputs, three routes, gated against
    float64 with the numpy fp32 product (+ fp32 exp) as the yardstick.  Under the exp also the largest per-entry RELATIVE error of the
    device and of the yardstick (the epilogue's __expf against an fp32 exp of the fp32 product): printed as "[exp-rel] op route device
    yardstick", nothing asserted on it beyond the gate.  Planted overflow / underflow entries: inf and 0 exactly, outside the gate."""
    nq, G, r, ld_q, ld_u, ld_s, pos, overflow = sl.GENERIC_CASES[case]
    pos_off, pos_idx = sl.positives(nq, G, pos, 100 + case)
    Q, U, planted = sl.generic_inputs(nq, G, r, 200 + case, exp, overflow and exp)
    I = _Inputs(Q, U, pos_off, pos_idx, ld_q, 0, ld_u, 0, ld_s, 0)
    S64, T64 = sl.scores64(Q, U, exp), sl.positives64(Q, U[pos_idx], pos_off, exp)
    with np.errstate(over="ignore"):
        raw32 = Q @ U.T
        S32 = np.exp(raw32) if exp else raw32
    rows = np.repeat(np.arange(nq), np.diff(pos_off))
    T32 = S32[rows, pos_idx]
    hole = np.zeros((nq, G), dtype=bool)
    for q, g in planted:
        hole[q, g] = True
    with np.errstate(over="ignore"):
        want32 = S64.astype(np.float32)
    if planted:
        assert np.isinf(want32[hole]).sum() == 4 and (want32[hole] == 0).sum() == 4
    items = []
    for route in ROUTES:
        for tail in ((False, True) if route == "mfma" else (False,)):
            S = _score_block(I, route, exp, tail)
            assert np.array_equal(S[hole], want32[hole]), "the planted inf / 0 pattern"
            fill = lambda a: np.where(hole, 0.0, a)
            items.append((f"S [{route} tail {int(tail)} exp {exp}]", fill(S), fill(S64), fill(S32)))
            if exp:
                rel = lambda a: float(np.max(np.abs(fill(a) - fill(S64)) / np.where(hole, 1.0, S64)))
                print(f"[exp-rel] txe_score_block {route} {rel(S):.3e} {rel(S32):.3e}")
        thr = _score_positives(I, route, exp)
        assert np.array_equal(thr, S[rows, pos_idx]), "txe_score_positives does not give the bits of txe_score_block"
        if I.n_pos:
            ph = hole[rows, pos_idx]
            fp = lambda a: np.where(ph, 0.0, a)
            items.append((f"thr [{route} exp {exp}]", fp(thr), fp(T64), fp(T32)))
    _gate("txe_score_block/positives", items)


# ---- (b) exact inputs: integer results, no tolerance ------------------------------------------------------------------------------------------
def _exact_params():
    out = [(c["name"], v) for c in sl.SCORE_CASES for v in c["variants"]]
    return out + [("wide", v) for v in sl.WIDE_CASE["variants"]]


def _exact_case(name, variant):
    if name == "wide":
        nq, G, p = sl.wide_shape(_cus())
        c = dict(sl.WIDE_CASE, nq=nq, G=G, ld_q=12, ld_u=12, off_q=0, off_u=0, ld_s=sl.round_up(G, 4) + 4, off_s=0, zero_from=None)
    else:
        c, p = next(c for c in sl.SCORE_CASES if c["name"] == name), 17
    pos_off, pos_idx = sl.positives(c["nq"], c["G"], c["pos"], 1, p)
    Q, U = sl.exact_inputs(c["nq"], c["G"], c["r"], 3, thin=variant == "exp", special=variant == "special", pos_off=pos_off, pos_idx=pos_idx, zero_from=c["zero_from"])
    return c, _Inputs(Q, U, pos_off, pos_idx, c["ld_q"], c["off_q"], c["ld_u"], c["off_u"], c["ld_s"], c["off_s"])


def _order_kept(raw, dev):
    """equal raw scores give equal bits; distinct raw scores keep their order (strictly)"""
    o = np.argsort(raw.ravel(), kind="stable")
    r, d = raw.ravel()[o], dev.ravel()[o].astype(np.float64)
    same = np.diff(r) == 0
    assert (np.diff(d)[same] == 0).all(), "equal raw scores with different exponentials"
    assert (np.diff(d)[~same] > 0).all(), "distinct raw scores merged or reordered by the exponential"


@pytest.mark.parametrize("name,variant", _exact_params(), ids=[f"{n}-{v}" for n, v in _exact_params()])
def test_exact_integer_results(name, variant):
    """all four entry points + txe_rank_finalize on exact inputs, three routes, both directions: see the module docstring, (b)"""
    c, I = _exact_case(name, variant)
    exp = int(variant == "exp")
    nq, G, n = I.nq, I.G, I.n_pos
    raw = sl.scores64(I.Q, I.U, False)                                     # exact; the exp is monotone: every integer result follows from raw
    rows = np.repeat(np.arange(nq), np.diff(I.pos_off))
    own = raw[rows, I.pos_idx]
    want32 = raw.astype(np.float32)
    ref = {}
    for larger in (1, 0):
        ref[larger] = dict(cnt=sl.counts(raw, I.pos_off, own, larger), ranks=sl.ranks(raw, I.pos_off, I.pos_idx, larger),
                           topk={k: sl.topk(raw, k, larger, sl.IDX_BASE) for k in sl.TOPK_KS})
        # the two definitions of a rank agree on the reference's side as well
        assert np.array_equal(sl.finalize(I.pos_off, own, ref[larger]["cnt"], larger), ref[larger]["ranks"])
    kinds = np.arange(n) % 5                                               # thresholds the test supplies, by kind
    with np.errstate(invalid="ignore"):
        mixed = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [own + 0.125, np.full(n, -np.inf), np.full(n, np.inf), np.full(n, np.nan)], own)
    S0 = None
    for route in ROUTES:
        S = _score_block(I, route, exp, tail=(route == "mfma"))
        if exp:
            _order_kept(raw, S)
            assert np.array_equal(S, S0) or S0 is None, "the routes' exponentials differ on exact raw scores"
            S0 = S
        else:
            assert np.array_equal(S, want32, equal_nan=True), f"scores not equal to float64 cast to fp32 [{route}]: {np.argwhere(~((S == want32) | (np.isnan(S) & np.isnan(want32))))[:8]}"
        thr = _score_positives(I, route, exp)
        assert np.array_equal(thr, S[rows, I.pos_idx], equal_nan=True), f"txe_score_positives != the staircase of txe_score_block [{route}]"
        for larger in (1, 0):
            R = ref[larger]
            cnt, td = _count(I, route, exp, thr, larger)                   # (non-exp: thr IS the exact own score, asserted above)
            assert np.array_equal(cnt, R["cnt"]), f"counts [{route} larger {larger}]: {np.flatnonzero(cnt != R['cnt'])[:8]}"
            assert np.array_equal(_finalize(I, td, cnt, larger), R["ranks"]), f"txe_rank_finalize [{route} larger {larger}]"
            if not exp and n:
                cnt2, _td = _count(I, route, 0, mixed, larger)
                assert np.array_equal(cnt2, sl.counts(raw, I.pos_off, mixed, larger)), f"counts, supplied thresholds [{route} larger {larger}]"
            for k in sl.TOPK_KS:
                idx, key = _topk(I, route, exp, larger, k, sl.IDX_BASE, with_key=(k != 5))
                wi, wk = R["topk"][k]
                assert np.array_equal(idx, wi), f"best {k} [{route} larger {larger}]: rows {np.flatnonzero((idx != wi).any(1))[:8]}"
                if key is not None:
                    if exp:
                        sk = sl.keys_of(S, larger)
                        wk = np.where(wi >= 0, np.take_along_axis(sk, np.maximum(wi - sl.IDX_BASE, 0), 1), -np.inf)
                    assert np.array_equal(key.astype(np.float64), wk), f"keys of the best {k} [{route} larger {larger}]"


def test_persistent_score_kernel():
    """txe_score_block with the tail workspace on the fp32 route at K = 160 and 8 row panels: whole rounds only, and whole rounds plus 16
    leftover tiles riding as whole tiles of the same launch (plain_k_order) -- exact inputs, bit-equal to float64, the launch name asserted"""
    for nq, G, r, rest in sl.persist_shapes(_cus()):
        plan = sl.persist_plan(nq, G, r, 4, 4, True, _cus())
        assert plan is not None and plan["rest"] == rest
        Q, U = sl.exact_inputs(nq, G, r, 5)
        I = _Inputs(Q, U, np.zeros(nq + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), r, 0, r, 0, sl.round_up(G, 4) + 4, 0)
        assert I.names("block", "mfma", True) == [plan["name"]]
        S = _score_block(I, "mfma", 0, tail=True)
        assert np.array_equal(S, sl.scores64(Q, U, False).astype(np.float32)), f"persistent kernel, {rest} leftover tiles"


# ---- (c) the rank and merge kernels alone -------------------------------------------------------------------------------------------------------
def _written_scores(nq, G, seed):
    rs = np.random.RandomState(seed)
    S = np.round(rs.randn(nq, G) * 3).astype(np.float32) / 2               # heavy ties
    for q in range(nq):
        for v in (np.nan, np.inf, -np.inf, -0.0, 0.0):
            S[q, rs.randint(0, G)] = v
    return rs, S


@pytest.mark.parametrize("case", range(len(sl.RANK_CASES)), ids=[f"{c[0]}x{c[1]}-ld{c[2]}+{c[3]}" for c in sl.RANK_CASES])
def test_rank_block_alone(case):
    """txe_rank_block on scores the test writes (ties, NaN, +-inf, -0.0 beside +0.0; a positive may be any of them), both directions,
    against the metric's definition; the ranks' NaN tail stays"""
    nq, G, ld, off, npos, _why = sl.RANK_CASES[case]
    rs, S = _written_scores(nq, G, 300 + case)
    pos_idx = np.concatenate([rs.choice(G, size=k, replace=False) for k in npos]).astype(np.int32)
    pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int32)
    if npos[-1] >= 2:                                                      # two positives of one query on -0.0 and +0.0, one on NaN
        S[nq - 1, pos_idx[-1]], S[nq - 1, pos_idx[-2]] = -0.0, 0.0
    if npos[-1] >= 3:
        S[nq - 1, pos_idx[-3]] = np.nan
    _b, sp = _laid(S, ld, off)
    n = int(pos_off[-1])
    offd, idxd = _up(pos_off), _up(pos_idx)
    for larger in (1, 0):
        rk = _nani(n + 8)
        _r, names = _profiled(lambda: _ok("txe_rank_block", sp, ld, nq, G, offd.data_ptr(), idxd.data_ptr(), rk.data_ptr(), larger, None, _st()))
        assert names == []
        _tail_intact(rk, n)
        assert np.array_equal(rk.cpu().numpy()[:n], sl.ranks(S, pos_off, pos_idx, larger)), (sl.RANK_CASES[case], larger)


def test_rank_finalize_alone():
    """txe_rank_finalize on thresholds and counts the test writes: ties, NaN, +-inf, -0.0 beside +0.0 among one query's thresholds; queries
    without positives first, in the middle and last; nq = 1"""
    rs = np.random.RandomState(9)
    for npos in ([0, 1, 8, 9, 0, 17, 130, 0], [5]):
        pos_off = np.concatenate([[0], np.cumsum(npos)]).astype(np.int32)
        n = int(pos_off[-1])
        thr = (np.round(rs.randn(n) * 2) / 2).astype(np.float32)
        thr[rs.choice(n, size=min(5, n), replace=False)] = (np.nan, np.inf, -np.inf, -0.0, 0.0)[:min(5, n)]
        cnt = rs.randint(0, 1000, n).astype(np.int32)
        td, cd, offd = _up(thr), _up(cnt), _up(pos_off)
        for larger in (1, 0):
            rk = _nani(n + 8)
            _ok("txe_rank_finalize", offd.data_ptr(), len(npos), td.data_ptr(), cd.data_ptr(), larger, rk.data_ptr(), _st())
            torch.cuda.synchronize()
            _tail_intact(rk, n)
            assert np.array_equal(rk.cpu().numpy()[:n], sl.finalize(pos_off, thr, cnt, larger))


@pytest.mark.parametrize("nq", sl.MERGE_NQ)
@pytest.mark.parametrize("cnt", sl.MERGE_CNTS)
def test_topk_merge_alone(cnt, nq):
    """txe_topk_merge on (key, idx) lists the test writes, every k from 1 to 8, idx_base 0 and 7, out_key given and NULL: heavy ties, +-inf,
    NaN keys (as -inf), -0.0 beside +0.0, real -inf keys beside empty slots (whose keys are NaN), rows with fewer than k real entries,
    a row of empty slots only, cnt == 0 (every slot -1 / -inf)"""
    rs = np.random.RandomState(cnt + nq)
    keys = (np.round(rs.randn(nq, cnt) * 2) / 2).astype(np.float32)
    idx = np.stack([rs.permutation(max(4 * cnt, 1))[:cnt] for _ in range(nq)]).astype(np.int32).reshape(nq, cnt)
    for q in range(nq):
        for v in (np.nan, np.inf, -np.inf, -np.inf, -0.0, 0.0)[:cnt]:
            keys[q, rs.randint(0, cnt)] = v
        real = [cnt, 3, 0, cnt // 2, 1][q % 5]                             # real entries of the row; the others are empty slots
        empty = rs.permutation(cnt)[:max(cnt - real, 0)]
        idx[q, empty], keys[q, empty[::2]] = sl.INT_MAX, np.nan
    kd, idd = _up(keys) if cnt else _nan(1), _up(idx) if cnt else _nani(1)
    for k in range(1, sl.TOPK_MAX + 1):
        for base, with_key in ((0, True), (7, True), (7, False)):
            oi, okey = _nani(nq * k + 8), (_nan(nq * k + 8) if with_key else None)
            _r, names = _profiled(lambda: _ok("txe_topk_merge", kd.data_ptr(), idd.data_ptr(), nq, cnt, k, base, oi.data_ptr(), _ptr(okey), _st()))
            assert names == ["topk_merge_kernel"]
            wi, wk = sl.merge(keys, idx, k, base)
            _tail_intact(oi, nq * k)
            assert np.array_equal(oi.cpu().numpy()[:nq * k].reshape(nq, k), wi), (cnt, nq, k, base)
            if with_key:
                _tail_intact(okey, nq * k)
                assert np.array_equal(okey.cpu().numpy()[:nq * k].reshape(nq, k).astype(np.float64), wk), (cnt, nq, k, base)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_launch_nothing():
    """every TXE_ERR_ARG / TXE_ERR_WORKSPACE condition txe.h states for the seven entry points: the code, no launch recorded, outputs and
    scratch still primed (floor_ws included: topk_floor_init_kernel records nothing, its writes would show there)"""
    nq, G, r, k = 5, 70, 12, 4
    pos_off, pos_idx = sl.positives(nq, G, "one", 2)
    Q, U = sl.exact_inputs(nq, G, r, 4)
    I = _Inputs(Q, U, pos_off, pos_idx, r, 0, r, 0, 72, 0)
    n, tiles = I.n_pos, sl.topk_tiles(G)
    S, thr, cnt, rk = _nan(nq * 72), _nan(n), _nani(n), _nani(n)
    pk, pi, fl, oi, okey = _nan(nq * tiles * k), _nani(nq * tiles * k), _nani(nq), _nani(nq * k), _nan(nq * k)
    sws = _nan(1 << 20)
    planes = I.planes().data_ptr()
    full = _L().call("txe_score_split_ws_bytes", nq, G, r)
    full_p = _L().call("txe_score_split_ws_bytes", nq, n, r)
    qonly = sl.round_up(_L().call("txe_split_packed_bytes", nq, r), 256)
    st, off = _st(), I.offd.data_ptr()
    A, W = sl.ERR_ARG, sl.ERR_WORKSPACE

    def block(Qp=I.Qp, ld_q=r, nq_=nq, Up=I.Up_, ld_u=r, G_=G, r_=r, Sp=S.data_ptr(), ld_s=72, sw=None, swb=0, upk=None):
        return lambda: _rc("txe_score_block", Qp, ld_q, nq_, Up, ld_u, G_, r_, 0, Sp, ld_s, None, 0, sw, swb, upk, st)

    def posv(Qp=I.Qp, ld_q=r, nq_=nq, Up=I.Pp, ld_u=r, n_=n, r_=r, offp=off, tp=thr.data_ptr(), sw=None, swb=0):
        return lambda: _rc("txe_score_positives", Qp, ld_q, nq_, Up, ld_u, n_, r_, 0, offp, tp, sw, swb, st)

    def count(Qp=I.Qp, ld_q=r, nq_=nq, Up=I.Up_, ld_u=r, G_=G, r_=r, offp=off, tp=thr.data_ptr(), cp=cnt.data_ptr(), sw=None, swb=0, upk=None):
        return lambda: _rc("txe_score_count_block", Qp, ld_q, nq_, Up, ld_u, G_, r_, 0, offp, tp, 1, cp, sw, swb, upk, st)

    def topk(Qp=I.Qp, ld_q=r, nq_=nq, Up=I.Up_, ld_u=r, G_=G, r_=r, k_=k, pkp=pk.data_ptr(), pip=pi.data_ptr(), flp=fl.data_ptr(), oip=oi.data_ptr(), sw=None, swb=0, upk=None):
        return lambda: _rc("txe_score_topk_block", Qp, ld_q, nq_, Up, ld_u, G_, r_, 0, 1, k_, 0, pkp, pip, flp, oip, okey.data_ptr(), sw, swb, upk, st)

    def mrg(kp=pk.data_ptr(), ip=pi.data_ptr(), nq_=nq, cnt_=tiles * k, k_=k, oip=oi.data_ptr()):
        return lambda: _rc("txe_topk_merge", kp, ip, nq_, cnt_, k_, 0, oip, okey.data_ptr(), st)

    def rankb(Sp=S.data_ptr(), nq_=nq, G_=G, offp=off, ip=I.idxd.data_ptr(), rp=rk.data_ptr()):
        return lambda: _rc("txe_rank_block", Sp, 72, nq_, G_, offp, ip, rp, 1, None, st)

    def fin(offp=off, nq_=nq, tp=thr.data_ptr(), cp=cnt.data_ptr(), rp=rk.data_ptr()):
        return lambda: _rc("txe_rank_finalize", offp, nq_, tp, cp, 1, rp, st)

    sp = sws.data_ptr()
    cases = [
        ("block nq < 0", block(nq_=-1), A), ("block G < 0", block(G_=-1), A), ("block r < 1", block(r_=0), A), ("block ld_u < r", block(ld_u=r - 1), A),
        ("block ld_q < r", block(ld_q=r - 1), A), ("block ld_s < G", block(ld_s=G - 1), A), ("block NULL Q", block(Qp=None), A), ("block NULL U", block(Up=None), A),
        ("block NULL S", block(Sp=None), A), ("block sws short", block(sw=sp, swb=full - 1), W), ("block sws short, u_packed", block(sw=sp, swb=qonly - 1, upk=planes), W),
        ("block ld_q < r, sws", block(ld_q=r - 1, sw=sp, swb=full), A),
        ("positives nq < 0", posv(nq_=-1), A), ("positives n_pos < 0", posv(n_=-1), A), ("positives r < 1", posv(r_=0), A), ("positives ld_u < r", posv(ld_u=r - 1), A),
        ("positives ld_q < r", posv(ld_q=r - 1), A), ("positives NULL Q", posv(Qp=None), A), ("positives NULL Up", posv(Up=None), A), ("positives NULL pos_off", posv(offp=None), A),
        ("positives NULL thr", posv(tp=None), A), ("positives sws short", posv(sw=sp, swb=full_p - 1), W),
        ("count nq < 0", count(nq_=-1), A), ("count G < 0", count(G_=-1), A), ("count r < 1", count(r_=0), A), ("count ld_u < r", count(ld_u=r - 1), A),
        ("count ld_q < r", count(ld_q=r - 1), A), ("count NULL Q", count(Qp=None), A), ("count NULL U", count(Up=None), A), ("count NULL pos_off", count(offp=None), A),
        ("count NULL thr", count(tp=None), A), ("count NULL counts", count(cp=None), A), ("count sws short", count(sw=sp, swb=full - 1), W),
        ("count sws short, u_packed", count(sw=sp, swb=qonly - 1, upk=planes), W),
        ("topk k = 0", topk(k_=0), A), ("topk k = 9", topk(k_=9), A), ("topk G = 0", topk(G_=0), A), ("topk nq < 0", topk(nq_=-1), A), ("topk r < 1", topk(r_=0), A),
        ("topk ld_u < r", topk(ld_u=r - 1), A), ("topk ld_q < r", topk(ld_q=r - 1), A), ("topk NULL Q", topk(Qp=None), A), ("topk NULL U", topk(Up=None), A),
        ("topk NULL part_key", topk(pkp=None), A), ("topk NULL part_idx", topk(pip=None), A), ("topk NULL floor_ws", topk(flp=None), A), ("topk NULL out_idx", topk(oip=None), A),
        ("topk sws short", topk(sw=sp, swb=full - 1), W), ("topk sws short, u_packed", topk(sw=sp, swb=qonly - 1, upk=planes), W),
        ("merge nq < 0", mrg(nq_=-1), A), ("merge cnt < 0", mrg(cnt_=-1), A), ("merge k = 0", mrg(k_=0), A), ("merge k = 9", mrg(k_=9), A), ("merge NULL keys", mrg(kp=None), A),
        ("merge NULL idx", mrg(ip=None), A), ("merge NULL out_idx", mrg(oip=None), A),
        ("rank_block nq < 0", rankb(nq_=-1), A), ("rank_block G < 0", rankb(G_=-1), A), ("rank_block NULL S", rankb(Sp=None), A), ("rank_block NULL pos_off", rankb(offp=None), A),
        ("rank_block NULL pos_idx", rankb(ip=None), A), ("rank_block NULL ranks", rankb(rp=None), A),
        ("finalize nq < 0", fin(nq_=-1), A), ("finalize NULL pos_off", fin(offp=None), A), ("finalize NULL thr", fin(tp=None), A), ("finalize NULL counts", fin(cp=None), A),
        ("finalize NULL ranks", fin(rp=None), A),
    ]
    for what, fn, code in cases:
        rc, names = _profiled(fn)
        assert rc == code and names == [], (what, rc, names)
    for t in (S, thr, pk, okey, sws):
        assert bool(torch.isnan(t).all()), "a rejected call wrote"
    for t in (cnt, rk, pi, fl, oi):
        assert bool((t == NANI).all()), "a rejected call wrote"
    # a single query has no pitch: ld_q and ld_s are not looked at
    I1 = _Inputs(Q[:1], U, np.array([0, 0], dtype=np.int32), np.zeros(0, dtype=np.int32), r, 0, r, 0, 72, 0)
    S1 = _nan(72)
    _ok("txe_score_block", I1.Qp, 0, 1, I1.Up_, r, G, r, 0, S1.data_ptr(), 0, None, 0, None, 0, None, st)
    torch.cuda.synchronize()
    assert np.array_equal(S1.cpu().numpy()[:G], sl.scores64(Q[:1], U, False)[0].astype(np.float32))
    # empty blocks are TXE_OK and launch nothing
    for what, fn in (("block nq 0", block(nq_=0)), ("block G 0", block(G_=0)), ("positives nq 0", posv(nq_=0)), ("positives n_pos 0", posv(n_=0)), ("count nq 0", count(nq_=0)),
                     ("count G 0", count(G_=0)), ("topk nq 0", topk(nq_=0)), ("merge nq 0", mrg(nq_=0)), ("rank_block nq 0", rankb(nq_=0)), ("finalize nq 0", fin(nq_=0))):
        rc, names = _profiled(fn)
        assert rc == 0 and names == [], (what, rc, names)
    assert bool(torch.isnan(S).all()) and bool((fl == NANI).all())
