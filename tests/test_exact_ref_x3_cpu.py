"""The bit-exact checker of tests/test_hip_exact_x3.py has teeth (no GPU needed): every case of the GPU file meets its preconditions, an
honest CPU model of a split-precision kernel passes assert_bits_equal / assert_stats_exact, and six models with ONE defect each at
2^-17 or 2^-18 of one operand are rejected."""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as E

B, CIN, COUT, HW = 2, 64, 96, (5, 7)           # two 32-channel chunks: K is short enough for BOTH operands to be wide


@pytest.fixture(scope="module")
def case():
    """1x1 with bias over two chunks, planes in, planes out, statistics: x and w both integers of 9 bits (256 .. 511, an odd one has
    lo = +-1), so that x_lo w_hi, x_hi w_lo AND the dropped x_lo w_lo are all non-zero, 64 x 511 x 511 = 1.67e7 stays below 2^24, and
    the sums reach 2^22: the OUT_SPLIT store drops a third part on most outputs."""
    g = E.gen(23)
    sgn = lambda s: 2.0 * torch.randint(0, 2, s, generator=g) - 1.0
    x = torch.randint(256, 512, (B, CIN, *HW), generator=g).double() * sgn((B, CIN, *HW))
    w = torch.randint(256, 512, (COUT, CIN, 1, 1), generator=g).double() * sgn((COUT, CIN, 1, 1))
    b = E.ints(g, (COUT,), -8, 8)
    E.check_exact(E.x3_margin(x, w, b) + (E.split_hi_lo(x)[1].abs().max() * E.split_hi_lo(w)[1].abs().max() * CIN).item())   # (room for the defect's term too)
    E.check_lo_share(x, 0.25, "x")
    E.check_lo_share(w, 0.25, "w")
    v = E.conv_x3_ref(x, w) + b.view(1, -1, 1, 1)
    E.check_out_split(v)
    assert E.split_profile(v)[1] > 0.5
    return dict(x=x, w=w, b=b, v=v)


def model(c, trunc_lo=False, drop_xlo_last_chunk=False, add_lolo=False, lo_channel_off=False, lo_from_rounded=False, stats_after_split=False):
    """A CPU model of a split kernel: per 32-channel chunk the three products, bias, the plane store, statistics of v; the keyword
    arguments switch single defects on.  Returns (hi plane, lo plane, statistics [B][2])."""
    xh, xl = E.split_hi_lo(c["x"])
    wh, wl = E.split_hi_lo(c["w"])
    if lo_channel_off:                              # the lo plane read one channel off (the hi plane in place)
        xl = xl.roll(1, 1)
    acc = torch.zeros(B, COUT, *HW, dtype=torch.float64)
    for c0 in range(0, CIN, 32):
        s = slice(c0, c0 + 32)
        acc = acc + F.conv2d(xh[:, s], wl[:, s]) + F.conv2d(xh[:, s], wh[:, s])
        if not (drop_xlo_last_chunk and c0 + 32 == CIN):
            acc = acc + F.conv2d(xl[:, s], wh[:, s])
        if add_lolo:
            acc = acc + F.conv2d(xl[:, s], wl[:, s])
    v = acc + c["b"].view(1, -1, 1, 1)
    hi, lo = (E.trunc_split if trunc_lo else E.split_hi_lo)(v)
    if lo_from_rounded:                             # lo = bf16(v' - hi) with v' the already rounded value: nothing is left for it
        lo = E.rne_bf16(E.rne_bf16(v).double() - hi).double()
    counted = hi + lo if stats_after_split else v
    return hi.float(), lo.float(), torch.stack([counted.flatten(1).sum(1), (counted ** 2).flatten(1).sum(1)], 1)


def check(c, got):
    hi, lo = E.store_split(c["v"])
    E.assert_bits_equal(got[0], hi.float(), "hi plane")
    E.assert_bits_equal(got[1], lo.float(), "lo plane")
    E.assert_stats_exact(got[2], c["v"], "model")


def test_honest_model_passes(case):
    check(case, model(case))
    # the reference is the documented algebra: x w without the x_lo w_lo term, which is not zero here
    xl, wl = E.split_hi_lo(case["x"])[1], E.split_hi_lo(case["w"])[1]
    full = F.conv2d(case["x"], case["w"], case["b"])
    assert torch.equal(full - F.conv2d(xl, wl), case["v"]) and (full != case["v"]).double().mean() > 0.9


DEFECTS = {
    "lo plane truncated toward zero": (dict(trunc_lo=True), "elements differ"),
    "x_lo w_hi dropped in the last 32-channel chunk": (dict(drop_xlo_last_chunk=True), "elements differ"),
    "x_lo w_lo added": (dict(add_lolo=True), "elements differ"),
    "lo plane read one channel off": (dict(lo_channel_off=True), "elements differ"),
    "OUT_SPLIT lo formed from an already rounded v": (dict(lo_from_rounded=True), "lo plane: .* elements differ"),
    "statistics counted from hi + lo": (dict(stats_after_split=True), "statistics"),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_checker_rejects_a_defective_model(case, name):
    kw, msg = DEFECTS[name]
    with pytest.raises(AssertionError, match=msg):
        check(case, model(case, **kw))


def test_truncated_input_split_is_caught_on_wide3_data():
    """A kernel that splits fp32 itself and truncates the lo plane: invisible on 10-bit integers, caught on the wide3 set."""
    import test_hip_exact_x3 as T
    g = E.gen(5)
    x, w = T.wide3_x(g, (1, 32, 4, 6)), E.ints(g, (8, 32, 1, 1), -1, 1, density=0.5)
    E.check_exact(E.x3_margin(x, w))
    assert not torch.equal(E.conv_x3_ref(x, w, split=E.trunc_split), E.conv_x3_ref(x, w))
    x10 = T.wide(g, (1, 32, 4, 6), 1023)
    assert torch.equal(E.conv_x3_ref(x10, w, split=E.trunc_split), E.conv_x3_ref(x10, w))


def test_split_helpers():
    v = torch.tensor([257.0, 259.0, 65537.0, 131329.0, 131075.0, 3.0, -65537.0, 0.0], dtype=torch.float64)
    hi, lo = E.split_hi_lo(v)
    # 257 = 256 + 1; 259 -> 260 - 1 (tie to even); 65537 = 65536 + 1; 131329 = 131072 + 257 -> lo 256 (tie to even), a third part of 1 is dropped;
    # 131075 = 131072 + 3
    assert hi.tolist() == [256.0, 260.0, 65536.0, 131072.0, 131072.0, 3.0, -65536.0, 0.0]
    assert lo.tolist() == [1.0, -1.0, 1.0, 256.0, 3.0, 0.0, -1.0, 0.0]
    assert E.trunc_split(v)[1].tolist() == lo.tolist()                                     # (nothing to truncate: every lo here is exact or a tie down)
    t = torch.tensor([131072.0 + 259.0], dtype=torch.float64)                               # lo = 259: rounds to 260, truncates to 258
    assert E.split_hi_lo(t)[1].item() == 260.0 and E.trunc_split(t)[1].item() == 258.0
    s_lo, s_drop, ties_hi, ties_lo = E.split_profile(v)
    assert (s_lo, s_drop, ties_hi, ties_lo) == (6 / 8, 1 / 8, 2, 1)
    ph, pl = E.store_split(v)
    assert ph.dtype == pl.dtype == torch.bfloat16 and torch.equal(ph.double(), hi) and torch.equal(pl.double(), lo)
    with pytest.raises(AssertionError):
        E.split_hi_lo(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))
    with pytest.raises(AssertionError, match="widen"):
        E.check_out_split(torch.arange(1000.0, dtype=torch.float64))                       # ten bits: lo != 0 often, but nothing is dropped
    with pytest.raises(AssertionError, match="wide3"):
        E.check_wide3(torch.arange(-(1 << 16), 1 << 16, 7).double())                       # +-2^16: 16 bits, no third part at all
    # a GroupNorm gain is folded into w before the split: 771 * 0.5 = 385.5 = 386 - 0.5
    x, w, gamma = torch.ones(1, 1, 1, 1, dtype=torch.float64), torch.full((1, 1, 1, 1), 771.0, dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64)
    assert E.conv_x3_ref(x, w, gamma=gamma).item() == 385.5
    # the margin counts the three magnitude sums in the unit of the smallest product of parts
    assert E.x3_margin(x * 3, w) == 3 * 772 + 3 * 1 and E.x3_margin(x * 3, w, gamma=gamma, unit=0.5) == 2 * (3 * 386 + 3 * 0.5)
    with pytest.raises(AssertionError, match="unit"):
        E.x3_margin(x * 3, w, gamma=gamma, unit=1.0)


def test_every_gpu_case_meets_its_preconditions():
    """The builders of tests/test_hip_exact_x3.py assert margin, lo shares, dropped third parts, ties and statistics bounds themselves."""
    import test_hip_exact_x3 as T
    assert T.all_cpu_cases() >= 70
