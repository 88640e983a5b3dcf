"""The bit-exact checker of tests/test_hip_exact.py has teeth (no GPU needed): assert_bits_equal accepts an honest CPU model of a
bf16 convolution kernel and rejects seven defective ones; every case of the GPU file meets its preconditions; the GELU table and
polynomial of the bf16 epilogue, recomputed here as the source builds them, stay within the bounds their comments state."""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as E

SHAPE, COUT = (2, 96, 8, 64), 192


@pytest.fixture(scope="module")
def case():
    """3x3 pad 1 with the nine-class GroupNorm fold, bias and a residual on integer data, at the shape of
    test_conv3x3_halo_matches_conv2d[(2, 96, 8, 64), cout 192]."""
    B, Cin, Hh, Ww = SHAPE
    g = E.gen(11)
    a, mean, gamma, beta = E.gn_numbers(g, B, Cin)
    a, mean = a[:, 0], mean[:, 0]
    x, w, b = E.ints(g, SHAPE, -4, 4), E.ints(g, (COUT, Cin, 3, 3), -2, 2), E.ints(g, (COUT,), -8, 8)
    r = E.ints(g, (B, COUT, Hh, Ww), -16, 16)
    E.check_exact(E.conv_fold_margin(x, w, b, gamma, beta, a, mean, r))
    pre = E.conv_fold_ref(x, w, b, gamma, beta, a, mean)
    E.check_rounding(pre + r)
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, a=a, mean=mean, r=r, pre=pre, want=E.rne_bf16(pre + r))


def model(c, store=E.rne_bf16, chunk_round=False, drop_tap=False, corner_class=False, double_round=False, drop_bias=None, swap=None):
    """A CPU model of the kernel: chunks of 32 input channels accumulated in turn, fold, residual, store; the keyword arguments
    switch single defects on."""
    x, w, gamma, beta, a, mean, b = c["x"], c["w"], c["gamma"], c["beta"], c["a"], c["mean"], c["b"]
    B, Cin, Hh, Ww = x.shape
    wg = w * gamma.view(1, -1, 1, 1)
    acc = torch.zeros(B, w.shape[0], Hh, Ww, dtype=torch.float64)
    for c0 in range(0, Cin, 32):
        acc = acc + F.conv2d(x[:, c0:c0 + 32], wg[:, c0:c0 + 32], None, padding=1)
        if chunk_round:
            acc = acc.float().bfloat16().double()
    if drop_tap:                                   # tap (0, 0) of input channel 5 missing at ONE pixel (the first whose input there is +-4)
        bb, yy, xx = (x[:, 5, :-1, :-1].abs() == 4).nonzero()[0].tolist()
        acc[bb, :, yy + 1, xx + 1] -= wg[:, 5, 0, 0] * x[bb, 5, yy, xx]
    if b is not None and drop_bias is not None:
        b = b.clone()
        b[drop_bias] = 0.0
    t1 = E.border_maps(w, beta, Hh, Ww) + b.view(-1, 1, 1)
    t2 = E.border_maps(w, gamma, Hh, Ww)
    if corner_class:                               # the corner pixel takes the shift row of the top edge next to it
        t1, t2 = t1.clone(), t2.clone()
        t1[:, 0, 0], t2[:, 0, 0] = t1[:, 0, 1], t2[:, 0, 1]
    a4, m4 = a.view(B, 1, 1, 1), mean.view(B, 1, 1, 1)
    v = a4 * acc + (t1[None] - a4 * m4 * t2[None])
    if double_round:
        v = E.rne_bf16(v).double()                 # rounded once before the residual, once more at the store
    out = store(v + c["r"])
    if swap is not None:
        out = out.clone()
        out[:, [swap[0], swap[1]]] = out[:, [swap[1], swap[0]]]
    return out


def test_honest_model_passes(case):
    E.assert_bits_equal(model(case), case["want"], "honest model")
    # and the fold algebra is GroupNorm followed by the convolution: conv((a x - a mean) gamma + beta, zero padded) + bias
    xn = (case["a"].view(-1, 1, 1, 1) * (case["x"] - case["mean"].view(-1, 1, 1, 1))) * case["gamma"].view(1, -1, 1, 1) + case["beta"].view(1, -1, 1, 1)
    assert torch.equal(F.conv2d(xn, case["w"], case["b"], padding=1), case["pre"])
    # fp32 F.conv2d reproduces the float64 integers: the premise of the whole method, on the CPU
    assert torch.equal(F.conv2d(case["x"].float(), case["w"].float(), None, padding=1).double(), F.conv2d(case["x"], case["w"], None, padding=1))


DEFECTS = {
    "truncating store": dict(store=E.trunc_bf16),
    "accumulator rounded to bf16 after every 32-channel chunk": dict(chunk_round=True),
    "one tap dropped at one pixel": dict(drop_tap=True),
    "corner pixel with an edge-class shift row": dict(corner_class=True),
    "rounded before the residual and again at the store": dict(double_round=True),
    "bias dropped on one channel": dict(drop_bias=77),
    "two output channels swapped inside one 8-channel group": dict(swap=(42, 45)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_checker_rejects_a_defective_model(case, name):
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_bits_equal(model(case, **DEFECTS[name]), case["want"], name)


def test_checker_reports_coordinates(case):
    bad = case["want"].clone()
    bad[1, 5, 3, 60] += 2.0
    with pytest.raises(AssertionError, match=r"1 of \d+ elements differ.*\(1, 5, 3, 60, got"):
        E.assert_bits_equal(bad, case["want"], "one element")


def test_preconditions_reject_what_they_should():
    g = E.gen(3)
    x, w = E.ints(g, (2, 64, 7, 3), -4, 4), E.ints(g, (64, 64, 3, 3), -2, 2)
    with pytest.raises(AssertionError, match="widen"):                  # the issue's example: |v| stays near 256, nothing rounds
        E.check_rounding(F.conv2d(x, w, None, padding=1))
    with pytest.raises(AssertionError, match="2\\^24"):
        E.check_exact(E.exactness_margin(x * 4096, w * 64, pad=1))
    with pytest.raises(AssertionError):
        E.check_stats(F.conv2d(E.ints(g, (1, 64, 16, 16), -32, 32), w, None, padding=1))
    with pytest.raises(AssertionError):
        E.rne_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    v = torch.tensor([257.0, 258.0, 259.0, 256.0, 3.0], dtype=torch.float64)       # 257: tie to even (256), 259: tie to even (260)
    assert E.rne_bf16(v).tolist() == [256.0, 258.0, 260.0, 256.0, 3.0] and E.trunc_bf16(v).tolist() == [256.0, 258.0, 258.0, 256.0, 3.0]
    assert E.rounding_profile(v) == (0.4, 2)


def test_every_gpu_case_meets_its_preconditions():
    """The builders of tests/test_hip_exact.py assert margin, rounding share, ties and statistics bounds themselves."""
    import test_hip_exact as T
    assert T.all_cpu_cases() > 100


def test_gelu_table_and_polynomial_keep_their_documented_bounds():
    """gelu_tab8: T(a) = a Phi(-a) at the midpoint of every bf16 bucket of [2^-12, 8), 1920 entries, clamped outside; gelu_poly8: its
    twelve coefficients and t = 2a/4.5 - 1, in fp32.  Both over every finite bf16 input (the table also at both ends of every bucket
    as fp32 inputs) against 0.5 x (1 + erf(x / sqrt 2)) in float64: <= 6.63e-4 and <= 2.0e-5 absolute, as conv_halo3_common.hpp states."""
    tab = E.gelu_table()
    assert tab.numel() == 1920 == E.GELU_TAB_N
    x = E.all_bf16_values()
    assert x.numel() == 65536 - 2 * 128
    err_tab = (E.gelu_tab_f32(x, tab).double() - E.gelu64(x)).abs()
    # inside a bucket the error is largest at an end: the first and the last fp32 pattern of every bucket, both signs
    p = (torch.arange(1920) + E.GELU_TAB_BASE).to(torch.int64) << 16
    ends = torch.cat([p, p + 0xFFFF]).to(torch.int32).view(torch.float32)
    ends = torch.cat([ends, -ends])
    err_ends = (E.gelu_tab_f32(ends, tab).double() - E.gelu64(ends)).abs()
    err_poly = (E.gelu_poly_f32(x).double() - E.gelu64(x)).abs()
    tiny = x.abs() < 2.0 ** -12
    half = (E.gelu_tab_f32(x[tiny], tab).double() - x[tiny].double() / 2).abs().max().item()
    print("gelu_tab8: max error %.4e over bf16 inputs (at x = %g), %.4e at bucket ends; |result - x/2| below 2^-12: %.4e; gelu_poly8: %.4e (at x = %g)"
          % (err_tab.max().item(), x[err_tab.argmax()].item(), err_ends.max().item(), half, err_poly.max().item(), x[err_poly.argmax()].item()))
    assert err_tab.max().item() <= E.E_GELU_TAB and err_ends.max().item() <= E.E_GELU_TAB
    assert x[err_tab.argmax()].item() == -2.0
    assert half <= 1.23e-4
    assert err_poly.max().item() <= E.E_GELU_POLY
    # the documented figures are tight: a table read one bucket off at x = -2, or a tanh-GELU, would not pass
    assert err_tab.max().item() > 6.6e-4 and err_poly.max().item() > 1.9e-5
    tanh_gelu = 0.5 * x.double() * (1 + torch.tanh(0.7978845608028654 * (x.double() + 0.044715 * x.double() ** 3)))
    assert (tanh_gelu - E.gelu64(x)).abs().max().item() > E.E_GELU_POLY
