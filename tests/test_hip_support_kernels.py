"""The fp32 dense and layout kernels (csrc/misc.hip) and the recurrent product of ds_lstm_layer (csrc/lstm.hip) through the C ABI, on every
path a launcher takes.  Cases, references, restatements and defect models: tests/support_ref.py; tests/test_support_ref_cpu.py shows without a
GPU that every case meets its preconditions and that every defect model changes the expected tensor.

Exact comparisons are torch.equal against float64 (integer data, sum |x||w| + |bias| < 2^24: every fp32 partial sum is exact in any order).
Where a comparison is not exact the rule of tests/test_hip_timbre.py holds and no tolerance is a constant: the fp32 CPU restatement's
distance from float64 (conftest.rel_err) is measured in the same run and the device gets four times that distance; both figures are printed,
and appended to $DS_SUPPORT_PARITY_LOG when that is set (profiles/support_kernels_parity.txt keeps those of one green run).

Every input and output lives in a support_ref.slab: a view inside a NaN-filled allocation, some of them 4-byte but not 16-byte aligned.  A
stray write changes a guard word, a stray read that reaches a result shows as NaN.

Which case reaches which launcher branch:
  ds_linear, linear_mfma_kernel<NBT>     NBT 1: B = 1, 16;  NBT 2: B = 17, 32;  NBT 4: B = 33, 64 (and B = 40 at K = 768);  NBT 8: B = 65, 128, 129,
                                         259 — each with every O of {1, 15, 16, 17, 64, 65} (under a wave's tile, ragged, one block of four waves, a
                                         second block) and every K of {16, 96, 112, 384} (1, 6, 7, 24 steps around `#pragma unroll 6`)
    second bt0 trip                      B = 129 (its first row, row 128) and B = 259 (rows 128 .. 255)
    third bt0 trip, ragged               B = 259 (rows 256 .. 258); test_linear_rows_do_not_depend_on_the_batch reads rows of all three trips
    bias = NULL, xs = K + 16, y one float off 16 bytes: once or more with every NBT;  ys = O + 5 in every case
  ds_linear, linear_kernel (fallback)    K % 16 != 0: K = 1, 20, 70;  xs % 4 != 0: K = 32, xs = 33;  x misaligned: K = 32, x one float off;
                                         W misaligned: K = 32, W one float off — at B in {1, 5}, O in {1, 17}
  ds_linear act_in                       GELU, SILU at B = 33 (NBT 4) and B = 129 (NBT 8, two trips)
  ds_lstm_layer                          H = 16: no 128-deep trip, a one-step tail;  H = 128: one trip, no tail;  H = 144: one trip and a
                                         one-step tail;  H = 272: two trips and a tail;  B = 17, 33: ragged second and third sample tile;
                                         T = 1: h never read
  ds_nchw_to_nhwc, ds_nhwc_to_nchw       second grid pass: (B, C, Cp, H, W) = (2, 3, 8, 400, 328) and (B, C, Cs, H, W) = (2, 8, 16, 400, 328), both
                                         2,048 elements above 8192 x 256
  ds_dup_batch                           vector kernel: 16 and 4096 + 16 bytes with distinct buffers; its second grid pass: 64 MiB + 48;
                                         in-place vector kernel: the same sizes with dst == src;  hipMemcpyAsync fallback: 20 bytes (either
                                         form) and every size with src 4 bytes off;  partial overlaps refused on the host
  ds_activation                          n = 1, 255, 257: one pass;  n = 2048 x 256 + 3: a second pass of the capped grid
  ds_add_layernorm                       D = 1, 37 (under one stride of 256), 256, 257, 512, 1000 (ragged fourth stride)"""
import os

import pytest
import torch

import exact_ref as E
import support_ref as S
import timbre_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from test_hip_exact import gelu_fast_bound
from test_hip_timbre import _check

pytestmark = pytest.mark.gpu

ACTS = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "silu": L.ACT_SILU}
NANBITS = 0x7FC00000


def note(line):
    """Figures worth keeping (profiles/support_kernels_parity.txt): printed, and appended to $DS_SUPPORT_PARITY_LOG when that is set."""
    print(line)
    path = os.environ.get("DS_SUPPORT_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def rule(what, dev, f32, f64):
    """The measured tolerance rule: dev within 4 x (fp32 CPU restatement vs float64) of float64."""
    assert tuple(dev.shape) == tuple(f64.shape) and bool(torch.isfinite(dev).all()), what
    cpu, err = rel_err(f32, f64), rel_err(dev.cpu(), f64)
    note(f"{what}: device vs float64 {err:.3e}, fp32 CPU restatement vs float64 {cpu:.3e}")
    assert err <= 4 * cpu, (what, err, cpu)
    return err, cpu


def sync():
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def unchanged(view, src):
    """An input slab still holds what was uploaded, bit for bit (NaN columns included)."""
    assert torch.equal(bits(view).cpu(), bits(src.to(view.dtype)))


# ================================================================================================= ds_linear, exact
def _linear(x, xs, w, b, B, K, O, act, y, ys):
    L.call("ds_linear", x.data_ptr(), xs, w.data_ptr(), L.ptr(b), B, K, O, act, y.data_ptr(), ys, L.current_stream())


def _run_exact_linear(c):
    x, w = S.slab(c.x_full.float(), offset_floats=c.x_off), S.slab(c.w.float(), offset_floats=c.w_off)
    b = S.slab(c.b.float()) if c.b is not None else None
    y = S.nan_slab((c.B, c.ys), offset_floats=c.y_off)
    assert (x.data_ptr() % 16 == 0) == (c.x_off == 0) and (w.data_ptr() % 16 == 0) == (c.w_off == 0) and (y.data_ptr() % 16 == 0) == (c.y_off == 0)
    _linear(x, c.xs, w, b, c.B, c.K, c.O, L.ACT_NONE, y, c.ys)
    sync()
    S.check_guards(*(t for t in (x, w, b, y) if t is not None))
    unchanged(x, c.x_full.float())
    unchanged(w, c.w.float())
    E.assert_bits_equal(y[:, :c.O].cpu(), c.want, "ds_linear " + c.id)
    assert bool(torch.isnan(y[:, c.O:]).all()), "columns O .. ys - 1 were written"


MFMA = [S.linear_case(**a) for a in S.linear_mfma_args()]
FALLBACK = [S.linear_case(**a) for a in S.linear_fallback_args()]


@pytest.mark.parametrize("case", MFMA, ids=[c.id for c in MFMA])
def test_linear_mfma_exact(case):
    assert case.mfma and case.nbt == S.nbt_of(case.B)
    _run_exact_linear(case)


@pytest.mark.parametrize("case", FALLBACK, ids=[c.id for c in FALLBACK])
def test_linear_fallback_exact(case):
    assert not case.mfma
    _run_exact_linear(case)


# ================================================================================================= ds_linear, random data
def test_linear_rows_do_not_depend_on_the_batch():
    """Rows of the first, second and (ragged) third bt0 trip of a B = 259 call equal, bit for bit, the same row in a call of its own."""
    c = S.linear_random_case(259, 112, 65)
    x, w, b = S.slab(c.x), S.slab(c.w), S.slab(c.b)
    y = S.nan_slab((c.B, c.O))
    _linear(x, c.K, w, b, c.B, c.K, c.O, L.ACT_NONE, y, c.O)
    for row in (0, 15, 16, 127, 128, 258):
        y1 = S.nan_slab((1, c.O))
        _linear(x[row:row + 1], c.K, w, b, 1, c.K, c.O, L.ACT_NONE, y1, c.O)
        sync()
        S.check_guards(y1)
        assert torch.equal(y1[0], y[row]), row
    S.check_guards(x, w, b, y)
    rule("ds_linear B=259 K=112 O=65", y, torch.nn.functional.linear(c.x, c.w, c.b), torch.nn.functional.linear(c.x.double(), c.w.double(), c.b.double()))


@pytest.mark.parametrize("B,K,O", [(33, 96, 17), (129, 112, 65)])
@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_linear_act_in(act, B, K, O):
    """act_in on the NBT = 4 and NBT = 8 (two trips) paths: bit-identical to ds_activation followed by ds_linear without act_in (the hoisted
    form the engine uses), and within the rule of float64.  The restatement of GELU is gelu_fast's own formula (support_ref.gelu_fast_f32)."""
    c = S.linear_random_case(B, K, O)
    x, w, b = S.slab(c.x), S.slab(c.w), S.slab(c.b)
    y, y2, xa = S.nan_slab((B, O + 5)), S.nan_slab((B, O + 5)), S.nan_slab((B, K))
    _linear(x, K, w, b, B, K, O, ACTS[act], y, O + 5)
    L.call("ds_activation", x.data_ptr(), x.numel(), ACTS[act], xa.data_ptr(), L.current_stream())
    _linear(xa, K, w, b, B, K, O, L.ACT_NONE, y2, O + 5)
    sync()
    S.check_guards(x, w, b, y, y2, xa)
    assert torch.equal(y[:, :O], y2[:, :O]) and bool(torch.isnan(y[:, O:]).all()) and bool(torch.isnan(y2[:, O:]).all())
    f32, f64 = S.linear_act_refs(c, act)
    rule(f"ds_linear act_in={act} B={B} K={K} O={O}", y[:, :O], f32, f64)


# ================================================================================================= ds_lstm_layer
@pytest.mark.parametrize("H,B,T", S.LSTM_SHAPES)
def test_lstm_layer_trip_and_tail(H, B, T):
    c = S.lstm_case(H, B, T)
    hs64, last64 = R.lstm_layer(c.pre.double(), c.w_hh)
    hs32, last32 = R.lstm_layer(c.pre, c.w_hh)
    pre, w = S.slab(c.pre, offset_floats=1), S.slab(c.w_hh)
    hs, h_last = S.nan_slab((B, T, H), offset_floats=1), S.nan_slab((B, H), offset_floats=3)
    ws = torch.full((L.load().ds_lstm_ws_floats(B, H),), S.NAN, device="cuda")
    L.call("ds_lstm_layer", pre.data_ptr(), T * 4 * H, 4 * H, w.data_ptr(), B, T, H, hs.data_ptr(), h_last.data_ptr(), ws.data_ptr(), L.current_stream())
    sync()
    S.check_guards(pre, w, hs, h_last)
    unchanged(pre, c.pre)
    e1 = _check(f"ds_lstm_layer H={H} B={B} T={T} hs", hs, hs32, hs64)
    e2 = _check(f"ds_lstm_layer H={H} B={B} T={T} h_last", h_last, last32, last64)
    note(f"ds_lstm_layer H={H} B={B} T={T}: hs device vs float64 {e1[0]:.3e}, restatement {e1[1]:.3e}; h_last {e2[0]:.3e}, restatement {e2[1]:.3e}")
    assert torch.equal(h_last, hs[:, -1])


# ================================================================================================= layout converters
DT = ((False, L.DS_F32, torch.float32), (True, L.DS_BF16, torch.bfloat16))


def _to_nhwc(x, Cp, bf16, dt, tdt, off=0):
    B, C, H, W = x.shape
    xd = S.slab(x.float(), offset_floats=off)
    out = S.nan_slab((B, H, W, Cp), tdt, offset_floats=off)
    L.call("ds_nchw_to_nhwc", xd.data_ptr(), B, C, H, W, out.data_ptr(), Cp, dt, L.current_stream())
    sync()
    S.check_guards(xd, out)
    want = S.nhwc_expect(x, Cp, bf16)
    E.assert_bits_equal(out.cpu(), want, f"ds_nchw_to_nhwc {tuple(x.shape)} Cp={Cp} bf16={bf16}")
    assert bool((bits(out[..., C:]) == 0).all()), "pad channels are not exact (positive) zeros"


def _to_nchw(x, Cs, bf16, dt, off=0):
    B, C, H, W = x.shape
    src = S.nhwc_source(x, Cs, bf16)
    sd = S.slab(src, offset_floats=off)
    out = S.nan_slab((B, C, H, W), offset_floats=off)
    L.call("ds_nhwc_to_nchw", sd.data_ptr(), dt, B, C, Cs, H, W, out.data_ptr(), L.current_stream())
    sync()
    S.check_guards(sd, out)
    unchanged(sd, src)
    E.assert_bits_equal(out.cpu(), S.nchw_expect(src, C), f"ds_nhwc_to_nchw {tuple(x.shape)} Cs={Cs} bf16={bf16}")


@pytest.mark.parametrize("C,Cp", S.LAYOUT_CP)
def test_layout_converters_exact(C, Cp):
    """fp32: a copy; bf16: one round-to-nearest-even (data with ties), pad channels exact zeros; the way back with Cs = C and C + 8 (NaN in
    the channels behind C).  B = 3 runs one float off a 16-byte boundary."""
    for H, W in S.LAYOUT_HW:
        for B in S.LAYOUT_B:
            x = S.layout_input(B, C, H, W)
            for bf16, dt, tdt in DT:
                _to_nhwc(x, Cp, bf16, dt, tdt, off=B // 3)
                for Cs in (C, C + 8):
                    _to_nchw(x, Cs, bf16, dt, off=B // 3)


@pytest.mark.parametrize("bf16,dt,tdt", DT, ids=["f32", "bf16"])
def test_layout_converters_second_grid_pass(bf16, dt, tdt):
    B, C, Cp, H, W = S.LAYOUT_BIG_FWD
    assert B * H * W * Cp > S.GRID_ELEMS
    _to_nhwc(S.layout_input(B, C, H, W), Cp, bf16, dt, tdt)
    B, C, Cs, H, W = S.LAYOUT_BIG_BACK
    assert B * C * H * W > S.GRID_ELEMS
    _to_nchw(S.layout_input(B, C, H, W), Cs, bf16, dt)


# ================================================================================================= ds_dup_batch
def _dup(src, dst, nbytes):
    L.call("ds_dup_batch", src.data_ptr(), dst.data_ptr(), nbytes, L.current_stream())


@pytest.mark.parametrize("form", ["distinct", "inplace", "src_off4"])
@pytest.mark.parametrize("nbytes", S.DUP_NBYTES)
def test_dup_batch_byte_exact(nbytes, form):
    words = S.dup_words(nbytes, "cuda")
    nw = words.numel()
    want = S.dup_expect(words)
    if form == "inplace":
        dst = S.slab(torch.cat([words, torch.full_like(words, NANBITS)]))
        src = dst
    else:
        src = S.slab(words, offset_floats=1 if form == "src_off4" else 0)
        dst = S.nan_slab((2 * nw,), torch.int32)
    assert S.dup_path(nbytes, src.data_ptr() % 16, form == "inplace") == ("memcpy" if nbytes % 16 or form == "src_off4" else "vector_inplace" if form == "inplace" else "vector")
    _dup(src, dst, nbytes)
    sync()
    S.check_guards(src, dst)
    assert torch.equal(dst, want)
    if form != "inplace":
        assert torch.equal(src, words)


def test_dup_batch_refuses_a_partial_overlap():
    """src == dst, or [src, src + n) and [dst, dst + 2n) disjoint; anything else is refused on the host and nothing is launched.  The two
    nearest allowed placements (src ending where dst begins, src beginning where dst ends) still copy."""
    n, nw = 256, 64
    words = S.dup_words(n, "cuda")
    base = S.slab(torch.cat([words, words + 1, words + 2, words + 3]))          # 4 n bytes
    before = base.clone()
    p = base.data_ptr()
    lib = L.load()
    for src, dst in ((p, p + 16), (p + n + 16, p), (p + n, p), (p + 2 * n - 16, p), (p + 16, p), (p + n - 16, p + n)):
        with pytest.raises(L.DsError, match="overlap"):
            L.call("ds_dup_batch", src, dst, n, L.current_stream())
        assert lib.ds_dup_batch(src, dst, n, L.current_stream()) == -1
    sync()
    assert torch.equal(base, before)
    S.check_guards(base)
    L.call("ds_dup_batch", p, p + n, n, L.current_stream())                       # src = [0, n), dst = [n, 3n)
    sync()
    assert torch.equal(base, torch.cat([words, words, words, words + 3]))
    base.copy_(before)
    L.call("ds_dup_batch", p + 2 * n, p, n, L.current_stream())                   # dst = [0, 2n), src = [2n, 3n)
    sync()
    assert torch.equal(base, torch.cat([words + 2, words + 2, words + 2, words + 3]))
    S.check_guards(base)


# ================================================================================================= ds_add_layernorm
@pytest.mark.parametrize("D", S.LN_D)
@pytest.mark.parametrize("B", S.LN_B)
def test_add_layernorm_against_float64(B, D):
    """Rows with |mean| / std from 0 to 1e3.  The restatement is the two-pass formula in torch fp32 (support_ref.layernorm_ref).  D = 1: the
    centred value is an exact zero on every route, restatement and device both give beta bit for bit (the allowance is zero)."""
    c = S.layernorm_case(B, D)
    off = B // 5
    a, r, g, be = S.slab(c.a, offset_floats=off), S.slab(c.r, offset_floats=off), S.slab(c.gamma, offset_floats=off), S.slab(c.beta, offset_floats=off)
    out = S.nan_slab((B, D), offset_floats=off)
    L.call("ds_add_layernorm", a.data_ptr(), r.data_ptr(), g.data_ptr(), be.data_ptr(), B, D, S.LN_EPS, out.data_ptr(), L.current_stream())
    sync()
    S.check_guards(a, r, g, be, out)
    rule(f"ds_add_layernorm B={B} D={D}", out, S.layernorm_ref(c, torch.float32), S.layernorm_ref(c, torch.float64))


# ================================================================================================= ds_activation
@pytest.mark.parametrize("n", S.ACT_N)
def test_activation(n):
    """Out of place and in place (the same bits); NONE a bit-exact copy; SILU and GELU by the rule.  act_apply's GELU is gelu_fast
    (csrc/common.hpp), not an exact-erf form: its restatement is support_ref.gelu_fast_f32, and every element is also held to the bound
    tests/test_hip_exact.py documents for gelu_fast (gelu_fast_bound)."""
    xc = S.act_input(n)
    off = 1 if n == 255 else 0
    x = S.slab(xc, offset_floats=off)
    for act in ("none", "silu", "gelu"):
        y, z = S.nan_slab((n,), offset_floats=off), S.slab(xc, offset_floats=off)
        L.call("ds_activation", x.data_ptr(), n, ACTS[act], y.data_ptr(), L.current_stream())
        L.call("ds_activation", z.data_ptr(), n, ACTS[act], z.data_ptr(), L.current_stream())
        sync()
        S.check_guards(x, y, z)
        unchanged(x, xc)
        assert torch.equal(bits(y), bits(z)), act
        if act == "none":
            assert torch.equal(bits(y).cpu(), bits(xc))
            continue
        rule(f"ds_activation {act} n={n}", y, S.act_f32(xc, act), S.act_f64(xc, act))
        if act == "gelu":
            err = (y.cpu().double() - S.act_f64(xc, act)).abs()
            bound = gelu_fast_bound(xc.double())
            k = (err / bound.clamp_min(1e-30)).argmax()
            note(f"ds_activation gelu n={n}: largest |got - gelu64| / E_fast = {(err[k] / bound[k].clamp_min(1e-30)).item():.3f} at x = {xc[k].item()!r}")
            assert bool((err <= bound).all())
