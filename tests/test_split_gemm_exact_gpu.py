"""The bf16 x 6 split GEMM (csrc/split_gemm.hip) against the one result its arithmetic can have: the set of six term pairs and the k-step tails.

A. Exact probe.  Operands v = s (H + Mi 2^-9 + L 2^-18), s = +-1, (H, Mi) from _HM, L in {0, 1}, zeros allowed; one operand dense, the other
   with at most 6 nonzeros per row (both orientations); bias and residual multiples of 2^-2 inside [-2, 2], PReLU slope 0.25.  Then
   * the kernel's round-to-nearest cut returns exactly (s H, s Mi 2^-9, s L 2^-18),
   * every product of two terms is a multiple of 2^-18,
   * every partial sum of an output element is bounded by sum|x||w| + |b| + |r| <= 6 * 3.006^2 + 4 < 64,
   so every partial sum is a multiple of 2^-18 below 2^6 -- 24 bits, exact in fp32 -- and the result does not depend on the order the matrix
   core adds in: the output must EQUAL the sum of the six pairs (PAIRS: the kernel's pair_a / pair_b table restated) plus the epilogue.  That
   is not the fp64 product of the operands: the three dropped pairs (mid*lo, lo*mid, lo*lo) make the two differ, after rounding
   to fp32, in a few per cent of the elements.  The unmarked CPU tests below assert the three conditions on the very operands the GPU cases use (the 256 x 256 form's operands
   are drawn on the device: their bound is asserted by construction, nonzeros per row x largest |v|^2).
   Cases per form (the form each launch took is parsed from the DF_GEMM_SPLIT_VERBOSE lines and asserted):
   * 128 x 128 (DF_GEMM_SPLIT_V=1): K = 32, 64, 96, 160, 416 (1, 2, 3, 5, 13 k32 steps: the single step, both break exits of the loop, long odd
     counts) x N = 128, 256 x M = 1, 127, 129, 300;
   * 256 x 128 (DF_GEMM_SPLIT_V=2): K = 384, 416, 448, 1056 (12, 13, 14, 33 steps: the odd counts reach the `if (nk & 1)` tail) x N = 128, 640 x
     M = 1, 255, 257, 700;
   * 256 x 256 (no switch): K = 384, 416, 448, N = 1024, M = 256 ceil(cu / 4) + 77 and 256 ceil(cu / 4) (cu: the card's compute units);
   * layouts on one K per form: in_ld > K with a channel offset, an output buffer wider than N with a channel offset (the columns outside
     stay untouched), both with a residual;
   * the rows16 fallback: a 256 x 256 launch whose output, or residual, starts one float past a 16-byte boundary reports 256x128, equals the
     expected values and the aligned launch's bits.
   Epilogues plain / ReLU / PReLU / residual + ReLU and launches without bias cycle over the cases.  A failure prints the difference in units of
   2^-18 and names the single change of the pair table (a pair left out, added twice, or multiplied from other planes) or the k32 step left
   out that reproduces the output (judged on the elements whose partial sums stay below 2^6 under that change too), or says "no single pair".
   Two checks on general values in the same children: scaling column k of x by 2^e(k) and of w by 2^-e(k), e in [-60, 60], changes no bit
   (the cut does not depend on the exponent; no term gets near a bf16 denormal), and a NaN in row M - 1 of a ragged M -- the row the padding
   rows re-read -- makes exactly row M - 1 of the output NaN.

B. The same K, M and layout cases once with randn operands against the fp64 product, by the rule of tests/test_split_gemm_engine_gpu.py:
   max|y - ref| / max|ref| at most 1.25 x the fp32-MFMA kernel's on the same operands (DF_GEMM_SPLIT_OFF=1) and below 2e-6, three repeats
   bit-identical.  The ratio is applied where the rule was established -- K >= 384 and M >= 252, the engine test's domain; below that
   (one row, one tile, a handful of k steps) both errors are a few final roundings of few elements and their ratio is noise: only the 2e-6
   cap applies there (_ratio_applies).

The development switches are read once per process: every variant is a child process (this file run as a script), never retried.

Measured on an MI355X (256 compute units: fill = 16 384 rows) with the kernels of commit 7d3616c (this module changes none of them):
* A: all 86 + 70 + 20 exact launches (128 x 128 / 256 x 128 / 256 x 256, the last with the two rows16 launches) equal the six-pair sum, first
  run.  The assumption under the probe -- the bf16 MFMA adds such products without loss while every partial sum fits 24 bits -- held at the
  full value set (largest sum|x||w| + |b| + |r| of the host-drawn cases 58.2); the set was not halved.
* The probe on wrong kernels (scratch builds, not committed): pair_b {0,2,1,0,1,0} -> {0,2,1,0,0,0} fails all 176 launches, each diagnosed
  "pair 4 (hi*mid) multiplied as hi*hi"; without the `if (nk & 1)` tail exactly the 38 launches of the 256 x 128 form with K = 416 / 1056 and
  the two rows16 launches (256 x 128 form, K = 416) fail, each diagnosed "k32 step 12 of 13 (32 of 33) left out"; every even count passes.
* Power-of-two scaling and the NaN row: no bit differs, on all three forms.  (The scales are exact powers of two built on the host; with torch.ldexp
  on the device the check failed.)
* B, max|y - ref| / max|ref|, split / fp32 kernel.  Where the ratio applies: 128 x 128 (2 cases) 3.7e-7 - 6.0e-7 / 3.9e-7 - 6.2e-7, worst
  ratio 0.96; 256 x 128 (27) 3.4e-7 - 1.05e-6 / 4.1e-7 - 1.19e-6, worst 1.05; 256 x 256 (9) 4.2e-7 - 9.0e-7 / 5.1e-7 - 9.5e-7, worst 0.95.
  Cap only (49 cases, in units of 1e-7, split / fp32; the ratio reaches 1.26 here, and 1.9 on another draw of the same shapes):
   128x128 K=32 N=128: M=1 0.75 / 1.64, M=127 0.96 / 1.13, M=129 1.27 / 1.98, M=300 0.89 / 1.12
   128x128 K=32 N=256: M=1 0.66 / 1.30, M=127 1.11 / 1.41, M=129 1.15 / 1.54, M=300 0.95 / 1.20
   128x128 K=64 N=128: M=1 1.26 / 1.52, M=127 2.32 / 2.73, M=129 1.51 / 2.43, M=300 1.21 / 1.51
   128x128 K=64 N=256: M=1 1.33 / 1.96, M=127 1.39 / 1.99, M=129 2.55 / 2.82, M=300 1.51 / 1.74
   128x128 K=96 N=128: M=1 1.84 / 2.98, M=127 1.84 / 2.34, M=129 2.15 / 2.97, M=300 1.63 / 2.44
   128x128 K=96 N=256: M=1 2.08 / 1.81, M=127 2.50 / 2.19, M=129 1.77 / 2.20, M=300 1.80 / 2.30
   128x128 K=160 N=128: M=1 2.89 / 3.78, M=127 3.09 / 3.48, M=129 3.69 / 3.69, M=300 2.54 / 2.38
   128x128 K=160 N=256: M=1 2.60 / 3.02, M=127 3.58 / 4.80, M=129 2.62 / 3.17, M=300 2.54 / 3.18
   128x128 K=416 N=128: M=1 4.01 / 3.19, M=127 4.38 / 5.84, M=129 5.99 / 6.48
   128x128 K=416 N=256: M=1 4.52 / 4.30, M=127 5.08 / 6.76, M=129 6.47 / 6.36
   128x128 K=96 N=256 layout in: M=300 1.93 / 1.90
   128x128 K=96 N=256 layout out: M=300 1.72 / 2.04
   128x128 K=96 N=256 layout inout: M=300 1.85 / 1.85
   256x128 K=384 N=128: M=1 3.25 / 3.05
   256x128 K=384 N=640: M=1 5.17 / 6.26
   256x128 K=416 N=128: M=1 3.54 / 3.76
   256x128 K=416 N=640: M=1 4.78 / 5.99
   256x128 K=448 N=128: M=1 2.07 / 3.23
   256x128 K=448 N=640: M=1 3.27 / 3.57
   256x128 K=1056 N=128: M=1 10.60 / 10.00
   256x128 K=1056 N=640: M=1 8.91 / 9.84
"""
import json
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("DF_GEMM_SPLIT_OFF", "DF_GEMM_SPLIT_BF16", "DF_GEMM_SPLIT_V", "DF_GEMM_SPLIT_VERBOSE", "DF_DEV_LIB")

# (plane of A, plane of B) of pair q, planes 0 hi / 1 mid / 2 lo: csrc/split_gemm.hip pair_a / pair_b
PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
_PLANE = ("hi", "mid", "lo")
_HM = ((1, 1), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3))
_VMAX = 3 + 3 * 2.0 ** -9 + 2.0 ** -18
_NNZ = 6
_KINDS = ("plain", "relu", "prelu", "resrelu")
_FORMS = {
    "128x128": dict(env={"DF_GEMM_SPLIT_V": "1"}, K=(32, 64, 96, 160, 416), N=(128, 256), M=(1, 127, 129, 300), lay=(96, 256, 300), gen="cpu"),
    "256x128": dict(env={"DF_GEMM_SPLIT_V": "2"}, K=(384, 416, 448, 1056), N=(128, 640), M=(1, 255, 257, 700), lay=(416, 640, 700), gen="cpu"),
    "256x256": dict(env={}, K=(384, 416, 448), N=(1024,), M=("fill+77", "fill"), lay=(416, 1024, "fill+77"), gen="cuda"),
}
# layouts: (in_ld - K, in_coff, out_ld - N, out_coff), offsets multiples of 4
_LAYOUTS = {"in": (24, 8, 0, 0), "out": (0, 0, 20, 12), "inout": (40, 12, 36, 4)}


def _rows(M, cu):
    """M of a case: `fill` is the fewest rows whose 256 x 256 tiles fill a card of cu compute units at N = 1024."""
    if isinstance(M, int):
        return M
    return 256 * (-(-cu // 4)) + (77 if M.endswith("+77") else 0)


def _cases(form):
    """The launches of one form, shared by part A (both orientations) and part B: dicts of K, N, M, kind, bias, layout."""
    f = _FORMS[form]
    out, i = [], 0
    for K in f["K"]:
        for N in f["N"]:
            for M in f["M"]:
                out.append(dict(form=form, K=K, N=N, M=M, i=i, layout=None))
                i += 1
    K, N, M = f["lay"]
    for lay in _LAYOUTS:
        out.append(dict(form=form, K=K, N=N, M=M, i=i, layout=lay))
        i += 1
    return out


def _kind(c, o):
    """Epilogue and bias of case c in orientation o (0 / 1): the four kinds and the launches without bias cycle over the cases."""
    if c["layout"] is not None:
        return "resrelu", True
    j = c["i"] + o
    return _KINDS[j % 4], j % 5 != 4


def _cid(c, tag):
    return f"{c['form']}-K{c['K']}-N{c['N']}-M{c['M']}-{c['layout'] or 'packed'}-{tag}"


def _seed(cid):
    return zlib.crc32(cid.encode())


def _ratio_applies(K, M):
    return K >= 384 and M >= 252


# ---- operands and the expected values (torch, either device)

def _lattice(rows, K, nnz, seed, device):
    """v [rows, K] fp32 and its designed terms (hi, mid, lo) in fp64; nnz: at most that many nonzeros per row, at positions drawn per row
    (one of them in the first and one in the last k32 step)."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda hi: torch.randint(0, hi, (rows, K), generator=g, device=device)
    hm = torch.tensor(_HM, dtype=torch.float64, device=device)[rnd(len(_HM))]
    s = rnd(2).double() * 2 - 1
    L = rnd(2).double()
    s = s * (rnd(16) != 0).double()                                            # zeros allowed
    if nnz is not None:
        pos = torch.randint(0, K, (rows, nnz), generator=g, device=device)
        pos[:, 0] = K - 32 + pos[:, 0] % 32                                     # every row reaches the last k32 step (the k loops' exits and tails)
        pos[:, 1] = pos[:, 1] % 32                                              # and the first
        s = s * torch.zeros(rows, K, dtype=torch.float64, device=device).scatter_(1, pos, 1.0)
    terms = (s * hm[..., 0], s * hm[..., 1] * 2.0 ** -9, s * L * 2.0 ** -18)       # the sign is shared: mixed signs would move the first cut
    return (terms[0] + terms[1] + terms[2]).float().contiguous(), terms


def _quarters(shape, seed, device):
    """multiples of 2^-2 in [-2, 2]"""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randint(-8, 9, shape, generator=g, device=device).double() / 4).float()


def _rne_bf16(v):
    """fp32 -> the nearest bf16 (ties to even) as fp32, by integer arithmetic on the bits (finite inputs)"""
    import torch
    b = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32)


def _cut3(v):
    """csrc/split_gemm.hip cut3 on the host: (hi, mid, lo), each difference exact in fp32"""
    hi = _rne_bf16(v)
    r = v - hi
    mid = _rne_bf16(r)
    return hi, mid, _rne_bf16(r - mid)


def _pair_sum(A, B, pairs=PAIRS):
    """sum over the pairs of A[a] @ B[b]^T in fp64 (A, B: term triples)"""
    return sum(A[a].double() @ B[b].double().t() for a, b in pairs)


def _epilogue(pre, bias, res, kind):
    import torch
    if bias is not None:
        pre = pre + bias.double()
    if res is not None:
        pre = pre + res.double()
    if kind in ("relu", "resrelu"):
        return torch.relu(pre)
    if kind == "prelu":
        return torch.where(pre > 0, pre, 0.25 * pre)
    return pre


def _exact_operands(c, o, cu, device):
    """Part A's operands of case c, orientation o (0: dense x, sparse w; 1: sparse x, dense w)."""
    cid = _cid(c, ("dense_x", "dense_w")[o])
    M, N, K = _rows(c["M"], cu), c["N"], c["K"]
    kind, has_bias = _kind(c, o)
    x, xt = _lattice(M, K, _NNZ if o == 1 else None, _seed(cid + "x"), device)
    w, wt = _lattice(N, K, _NNZ if o == 0 else None, _seed(cid + "w"), device)
    bias = _quarters((N,), _seed(cid + "b"), device) if has_bias else None
    res = _quarters((M, N), _seed(cid + "r"), device) if kind == "resrelu" else None
    return dict(id=cid, M=M, N=N, K=K, kind=kind, x=x, w=w, xt=xt, wt=wt, bias=bias, res=res)


def _check_conditions(op):
    """The three conditions the exactness argument needs, on one case's operands; returns the largest sum|x||w| + |b| + |r|."""
    import torch
    for v, t in ((op["x"], op["xt"]), (op["w"], op["wt"])):
        cut = _cut3(v)
        for got, want in zip(cut, t):
            assert torch.equal(got.double(), want), op["id"]                     # the cut returns the designed terms
        assert torch.equal(cut[0].double() + cut[1].double() + cut[2].double(), v.double()), op["id"]       # and they sum to the value
        assert torch.equal((t[0] + t[1] + t[2]).float().double(), t[0] + t[1] + t[2]), op["id"]             # the value is an fp32 number
    bound = op["x"].double().abs() @ op["w"].double().abs().t()
    if op["bias"] is not None:
        bound = bound + op["bias"].double().abs()
    if op["res"] is not None:
        bound = bound + op["res"].double().abs()
    assert float(bound.max()) < 64, (op["id"], float(bound.max()))
    pre = _epilogue(_pair_sum(op["xt"], op["wt"]), op["bias"], op["res"], "plain")
    assert torch.equal(torch.round(pre * 2 ** 18), pre * 2 ** 18), op["id"]      # multiples of 2^-18 (below 2^6: 24 bits)
    exp = _epilogue(_pair_sum(_cut3(op["x"]), _cut3(op["w"])), op["bias"], op["res"], op["kind"])
    assert torch.equal(exp.float().double(), exp), op["id"]                      # the expected values are fp32 numbers
    return float(bound.max())


@pytest.mark.parametrize("form", ["128x128", "256x128"])
def test_exact_operands_meet_the_conditions_of_the_exactness_argument(form):
    worst = 0.0
    for c in _cases(form):
        for o in (0, 1):
            worst = max(worst, _check_conditions(_exact_operands(c, o, 0, "cpu")))
    print(f"{form}: largest sum|x||w| + |b| + |r| = {worst:.3f}")
    assert worst < 64


def test_device_drawn_operands_are_bounded_by_construction():
    # the 256 x 256 form's operands are drawn on the device by the same _lattice: at most _NNZ nonzero products per output element
    assert _NNZ * _VMAX ** 2 + 2 + 2 < 64
    for o in (0, 1):          # the recipe itself, at a small M on the host
        c = dict(_cases("256x256")[1], M=77)
        op = _exact_operands(c, o, 0, "cpu")
        assert int(((op["x"] if o else op["w"]) != 0).sum(1).max()) <= _NNZ
        assert float(op["x"].abs().max()) <= _VMAX and float(op["w"].abs().max()) <= _VMAX
        _check_conditions(op)


def test_dropping_any_pair_changes_most_of_the_expected_values():
    import torch
    op = _exact_operands(_cases("256x128")[13], 0, 0, "cpu")          # K = 416
    full = _pair_sum(op["xt"], op["wt"])
    for q in range(6):
        changed = float((_pair_sum(op["xt"], op["wt"], PAIRS[:q] + PAIRS[q + 1:]) != full).double().mean())
        print(f"without pair {q}: {100 * changed:.0f} % of the elements change")
        assert changed > 0.5, (q, changed)
    nine = _pair_sum(op["xt"], op["wt"], [(a, b) for a in range(3) for b in range(3)])
    assert torch.equal(nine, op["x"].double() @ op["w"].double().t())
    differ = float((nine.float().double() != full).double().mean())           # the six-pair sum is not the fp32-rounded fp64 product
    print(f"fp64 product rounded to fp32 against the six-pair sum: {100 * differ:.1f} % of the elements differ")
    assert 0 < differ < 0.5


# ---- the child process (this file run as a script)

def _launch(x, w, K, bias, res, kind, in_coff=0, out=None, out_coff=0):
    import torch
    from densefusion_amd import ops
    M, N = x.shape[0], w.shape[0]
    pr = torch.tensor([0.25], device=x.device) if kind == "prelu" else None
    y = ops.conv2d_nhwc(x.view(1, M, 1, x.shape[1]), w.view(N, 1, 1, K), bias=bias, act={"plain": 0, "relu": 1, "resrelu": 1, "prelu": 2}[kind],
                        res=None if res is None else res.view(1, M, 1, N), prelu=pr, out=None if out is None else out.view(1, M, 1, out.shape[1]),
                        out_coff=out_coff, in_coff=in_coff, cin=K)
    return y.view(M, -1)


def _with_layout(c, x, N):
    """x inside a wider buffer (NaN around it) and a pre-filled output buffer, per the case's layout: x, in_coff, out, out_coff"""
    import torch
    if c["layout"] is None:
        return x, 0, None, 0
    dl, ic, do, oc = _LAYOUTS[c["layout"]]
    M, K = x.shape
    if dl:
        xb = torch.full((M, K + dl), float("nan"), device=x.device)
        xb[:, ic:ic + K] = x
        x = xb
    out = torch.full((M, N + do), -777.0, device=x.device) if do else None
    return x, ic, out, oc


def _take(y, out, oc, N):
    """the N result columns; asserts the rest of a wider buffer is untouched"""
    if out is None:
        return y, True
    keep = [i for i in range(out.shape[1]) if not oc <= i < oc + N]
    return out[:, oc:oc + N], bool((out[:, keep] == -777.0).all())


def _diagnose(y, exp, op, form, cid=None):
    """What is wrong with y: differences in units of 2^-18 and the single change of the pair table, or k32 step left out, that reproduces y."""
    import torch
    bad = (y.double() != exp).nonzero()
    g = torch.Generator().manual_seed(1)
    more = torch.stack([torch.randint(0, y.shape[0], (256,), generator=g), torch.randint(0, y.shape[1], (256,), generator=g)], 1).to(bad.device)
    m, n = torch.cat([bad[:256], more]).t()
    a = torch.stack([t.double() for t in _cut3(op["x"])])[:, m]          # [3, S, K]
    b = torch.stack([t.double() for t in _cut3(op["w"])])[:, n]
    nk = op["K"] // 32
    t = torch.einsum("ask,bsk->absk", a, b).view(3, 3, len(m), nk, 32).sum(-1)          # [plane of A, plane of B, sample, k32 step]
    tm = torch.einsum("ask,bsk->absk", a.abs(), b.abs()).view(3, 3, len(m), nk, 32).sum(-1)          # the products' magnitudes
    base = sum(t[pa, pb] for pa, pb in PAIRS)
    got = y[m, n].double()

    bias = op["bias"][n] if op["bias"] is not None else None
    res = op["res"][m, n] if op["res"] is not None else None
    extra = (bias.double().abs() if bias is not None else 0) + (res.double().abs() if res is not None else 0)
    wrong = torch.zeros(len(m), dtype=torch.bool, device=m.device)
    wrong[:min(256, len(bad))] = True

    def matches(pre, mag):          # pre, mag [S, nk]: a hypothesis' products and their magnitudes.  It has ONE fp32 result only where its partial
        sure = mag.sum(1) + extra < 64          # sums stay below 2^6: those elements decide, and some of them must be wrong ones
        return bool((sure & wrong).any()) and bool(((_epilogue(pre.sum(1), bias, res, op["kind"]) == got) | ~sure).all())
    mag = sum(tm[pa, pb] for pa, pb in PAIRS)
    found = []
    for q, (pa, pb) in enumerate(PAIRS):
        name = f"pair {q} ({_PLANE[pa]}*{_PLANE[pb]})"
        if matches(base - t[pa, pb], mag - tm[pa, pb]):
            found.append(name + " left out")
        if matches(base + t[pa, pb], mag + tm[pa, pb]):
            found.append(name + " added twice")
        for ra in range(3):
            for rb in range(3):
                if (ra, rb) != (pa, pb) and matches(base - t[pa, pb] + t[ra, rb], mag - tm[pa, pb] + tm[ra, rb]):
                    found.append(f"{name} multiplied as {_PLANE[ra]}*{_PLANE[rb]}")
    for s in range(nk):
        keep = torch.ones(nk, dtype=torch.float64, device=base.device)
        keep[s] = 0
        if matches(base * keep, mag * keep):
            found.append(f"k32 step {s} of {nk} left out")
    first = []
    for i in range(min(5, len(bad))):
        steps = sorted(set((torch.nonzero(op["x"][m[i]] * op["w"][n[i]]).flatten() // 32).tolist()))
        first.append(f"(m={int(m[i])}, n={int(n[i])}): {float((got[i] - exp[m[i], n[i]]) * 2 ** 18):+.6g} x 2^-18, nonzero products in k32 steps {steps}")
    return (f"{cid or op['id']} [{op['kind']}, form {form}]: {len(bad)} of {y.numel()} elements differ from the six-pair sum; "
            f"reproduced by: {'; '.join(found) if found else 'no single pair'}; " + "; ".join(first))


def _say(cid):
    sys.stderr.write(f"[case] {cid}\n")
    sys.stderr.flush()


def _child_exact(form, cu, dev):
    import torch
    res = []
    for c in _cases(form):
        for o in (0, 1):
            op = _exact_operands(c, o, cu, _FORMS[form]["gen"])
            op = {k: (v.to(dev) if torch.is_tensor(v) else tuple(t.to(dev) for t in v) if isinstance(v, tuple) else v) for k, v in op.items()}
            for v, t in ((op["x"], op["xt"]), (op["w"], op["wt"])):          # (the cut returns the designed terms: also on device-drawn operands)
                assert all(torch.equal(g.double(), want) for g, want in zip(_cut3(v), t)), op["id"]
            exp = _epilogue(_pair_sum(op["xt"], op["wt"]), op["bias"], op["res"], op["kind"])
            x, ic, out, oc = _with_layout(c, op["x"], op["N"])
            _say(op["id"])
            y, clean = _take(_launch(x, op["w"], op["K"], op["bias"], op["res"], op["kind"], ic, out, oc), out, oc, op["N"])
            torch.cuda.synchronize()
            ok = torch.equal(y.double(), exp)
            res.append(dict(id=op["id"], forms=[form], ok=ok, untouched=clean, msg="" if ok else _diagnose(y, exp, op, form)))
            if form == "256x256" and c["layout"] == "inout" and o == 0:
                # the rows16 fallback: output, then residual, one float past a 16-byte boundary
                M, N = op["M"], op["N"]
                for what in ("out", "res"):
                    flat = torch.full((M * N + 1,), -777.0, device=dev)
                    r2, o2 = op["res"], None
                    if what == "out":
                        o2 = flat[1:].view(M, N)
                    else:
                        flat[1:] = op["res"].flatten()
                        r2 = flat[1:].view(M, N)
                    assert (r2 if what == "res" else o2).data_ptr() % 16 == 4
                    _say(op["id"] + "-rows16-" + what)
                    y2 = _launch(op["x"], op["w"], op["K"], op["bias"], r2, op["kind"], out=o2)
                    torch.cuda.synchronize()
                    ok2 = torch.equal(y2.double(), exp)
                    res.append(dict(id=op["id"] + "-rows16-" + what, forms=["256x128"], ok=ok2, untouched=True, same_as_aligned=torch.equal(y2, y),
                                    msg="" if ok2 else _diagnose(y2, exp, op, "256x128", op["id"] + "-rows16-" + what)))
    return res


def _general_operands(c, cu, device):
    import torch
    cid = _cid(c, "g")
    M, N, K = _rows(c["M"], cu), c["N"], c["K"]
    g = torch.Generator(device=device).manual_seed(_seed(cid))
    kind, has_bias = _kind(c, 0)
    x = torch.randn(M, K, generator=g, device=device)
    w = torch.randn(N, K, generator=g, device=device) / K ** 0.5
    bias = torch.randn(N, generator=g, device=device) if has_bias else None
    res = torch.randn(M, N, generator=g, device=device) if kind == "resrelu" else None
    return dict(id=cid, M=M, N=N, K=K, kind=kind, x=x, w=w, bias=bias, res=res)


def _child_general(forms, cu, dev, expect_form):
    import torch
    res = []
    for form in forms:
        for c in _cases(form):
            op = _general_operands(c, cu, _FORMS[form]["gen"])
            op = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in op.items()}
            ref = _epilogue(op["x"].double() @ op["w"].double().t(), op["bias"], op["res"], op["kind"])
            outs = []
            _say(op["id"])
            for _ in range(3):
                x, ic, out, oc = _with_layout(c, op["x"], op["N"])
                y, clean = _take(_launch(x, op["w"], op["K"], op["bias"], op["res"], op["kind"], ic, out, oc), out, oc, op["N"])
                outs.append(y.clone())
            torch.cuda.synchronize()
            res.append(dict(id=op["id"], K=op["K"], M=op["M"], forms=[form] * 3 if expect_form else [], untouched=clean,
                            err=float((outs[0].double() - ref).abs().max() / ref.abs().max()), same=all(torch.equal(outs[0], o) for o in outs[1:])))
    return res


def _child_invariants(form, cu, dev):
    """general values: power-of-two scaling of the k columns changes no bit; a NaN row M - 1 reaches exactly row M - 1"""
    import torch
    K, N, M = _FORMS[form]["lay"]
    M = _rows(M, cu)
    g = torch.Generator().manual_seed(_seed(form + "inv"))
    x, w, bias = torch.randn(M, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** 0.5).to(dev), torch.randn(N, generator=g).to(dev)
    e = torch.randint(-60, 61, (K,), generator=g).tolist()
    up, down = (torch.tensor([2.0 ** (sg * k) for k in e], device=dev) for sg in (1, -1))          # exact powers of two (not the device's pow)
    xs, ws = (x * up).contiguous(), (w * down).contiguous()
    _say(form + "-invariants")
    y = _launch(x, w, K, bias, None, "plain").clone()
    ys = _launch(xs, ws, K, bias, None, "plain").clone()
    xn = x.clone()
    xn[M - 1] = float("nan")
    yn = _launch(xn, w, K, bias, None, "plain").clone()
    torch.cuda.synchronize()
    return dict(id=form + "-invariants", forms=[form] * 3, finite=bool(torch.isfinite(y).all()), ragged=M % 256 != 0,
                scaling_exact=torch.equal(xs * down, x) and torch.equal(ws * up, w), scaled_same=torch.equal(y, ys), scaled_differ=int((y != ys).sum()),
                nan_row=bool(torch.isnan(yn[M - 1]).all()), other_rows_same=torch.equal(yn[:M - 1], y[:M - 1]))


def _child_main(mode, form):
    import torch
    dev = torch.device("cuda")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    if mode == "fp32":
        out = dict(general=_child_general(list(_FORMS), cu, dev, False))
    else:
        out = dict(exact=_child_exact(form, cu, dev), general=_child_general([form], cu, dev, True), invariants=_child_invariants(form, cu, dev))
    print(json.dumps(out))


# ---- the GPU tests

def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not os.path.exists(os.path.join(ROOT, "densefusion_amd", "libdfusion_hip_dev.so")):
        pytest.skip("development library not built")


_RUNS = {}


def _child(mode, form=""):
    """One child per variant, run once (a failed child is not run again: its failure is kept)."""
    key = (mode, form)
    if key not in _RUNS:
        env = dict(os.environ, PYTHONPATH=ROOT)
        for k in _SWITCHES:
            env.pop(k, None)
        env.update({"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_VERBOSE": "1"})
        env.update({"DF_GEMM_SPLIT_OFF": "1"} if mode == "fp32" else dict(_FORMS[form]["env"], DF_GEMM_SPLIT_BF16="1"))
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), mode, form], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, timeout=240)
            assert out.returncode == 0, out.stderr[-3000:]
            took, cur = {}, None
            for line in out.stderr.splitlines():          # the forms each case's launches took
                if line.startswith("[case] "):
                    cur = took.setdefault(line[7:], [])
                elif line.startswith("[df-split] M="):
                    assert line.endswith("-> bf16 x 6"), (line, cur)
                elif line.startswith("[df-split]   form "):
                    cur.append(line.split()[-1])
            _RUNS[key] = (json.loads(out.stdout.strip().splitlines()[-1]), took)
        except Exception as e:          # kept, and raised again for every test that needs this child
            _RUNS[key] = e
    if isinstance(_RUNS[key], Exception):
        raise _RUNS[key]
    return _RUNS[key]


def _assert_forms(results, took):
    for r in results:
        print(f"{r['id']}: form {' '.join(took.get(r['id'], [])) or '-'}")
        assert took.get(r["id"], []) == r["forms"], (r["id"], took.get(r["id"]), r["forms"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(_FORMS))
def test_the_kernel_equals_the_six_pair_sum_bit_for_bit(form):
    _need_gpu()
    res, took = _child("split", form)
    _assert_forms(res["exact"], took)
    bad = [r["msg"] for r in res["exact"] if not r["ok"]]
    assert not bad, f"{len(bad)} of {len(res['exact'])} cases:\n" + "\n".join(bad[:12])
    assert all(r["untouched"] for r in res["exact"]), [r["id"] for r in res["exact"] if not r["untouched"]]
    rows16 = [r for r in res["exact"] if "same_as_aligned" in r]
    assert len(rows16) == (2 if form == "256x256" else 0) and all(r["same_as_aligned"] for r in rows16), rows16


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(_FORMS))
def test_power_of_two_scaling_changes_no_bit_and_a_nan_row_stays_in_its_row(form):
    _need_gpu()
    res, took = _child("split", form)
    r = res["invariants"]
    _assert_forms([r], took)
    assert r["finite"] and r["ragged"], r
    assert r["scaling_exact"] and r["scaled_same"], r
    assert r["nan_row"] and r["other_rows_same"], r


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(_FORMS))
def test_general_values_stay_inside_the_fp32_kernels_error_on_the_new_paths(form):
    _need_gpu()
    res, took = _child("split", form)
    fp32 = {r["id"]: r for r in _child("fp32")[0]["general"]}
    _assert_forms(res["general"], took)
    for s in res["general"]:
        f = fp32[s["id"]]
        rule = "ratio + cap" if _ratio_applies(s["K"], s["M"]) else "cap only"
        print(f"{s['id']}: split {s['err']:.2e}  fp32 {f['err']:.2e}  ({rule})")
    for s in res["general"]:
        f = fp32[s["id"]]
        assert s["same"] and f["same"] and s["untouched"] and f["untouched"], (s, f)
        assert s["err"] < 2e-6, s
        if _ratio_applies(s["K"], s["M"]):
            assert s["err"] <= 1.25 * f["err"], (s, f)


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
