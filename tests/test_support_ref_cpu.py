"""The inputs of tests/test_hip_support_kernels.py can tell a faulty kernel from a right one (no GPU needed).

Every case of tests/support_ref.py is built again here, which asserts its preconditions (fp32-exact operands, sum |x||w| + |bias| < 2^24,
the share of many-bit operand elements, distinct rows), and every defect model of that file is applied to every case where the fault can
show: on exact data the expected tensor must change (torch.equal is false), on tolerance data the result must move by at least ten times
the allowance the GPU test measures in the same run (four times the fp32 restatement's distance from float64).  Each defect model must show
in at least one case."""
import pytest
import torch

import exact_ref as E
import support_ref as S
from conftest import rel_errs


def rel_err(a, b):
    """Both error norms of the suite, the larger one — without conftest.rel_err's log: the figures here are deliberate faults, not parity."""
    return max(rel_errs(a, b))


# ------------------------------------------------------------------------------------------------ ds_linear
LINEAR = S.linear_cases()


def test_linear_covering_set():
    """Every O and every K with every NBT, both ends of every NBT, the variants with every NBT, the named single cases, and the fallback
    by each of its four conditions at B in {1, 5} and O in {1, 17}."""
    mf = [c for c in LINEAR if c.mfma]
    fb = [c for c in LINEAR if not c.mfma]
    assert len(mf) == len(S.linear_mfma_args()) and len(fb) == len(S.linear_fallback_args())
    for nbt, bs in ((1, (1, 16)), (2, (17, 32)), (4, (33, 64)), (8, (65, 128, 129, 259))):
        own = [c for c in mf if c.nbt == nbt]
        assert {c.B for c in own} - {40} == set(bs), nbt
        assert {c.O for c in own} >= {1, 15, 16, 17, 64, 65} and {c.K for c in own} >= {16, 96, 112, 384}, nbt
        assert any(c.b is None for c in own) and any(c.xs == c.K + 16 for c in own) and any(c.y_off == 1 for c in own), nbt
        assert {c.wide for c in own} == {"x", "w"}, nbt
    assert all(c.ys == c.O + 5 for c in LINEAR)
    assert any((c.B, c.K, c.O) == (259, 112, 65) for c in mf) and any((c.B, c.K, c.O) == (40, 768, 48) for c in mf)
    assert {c.K for c in fb if c.K % 16} == {1, 20, 70}
    assert any(c.K == 32 and c.xs == 33 for c in fb) and any(c.x_off == 1 and c.xs % 4 == 0 for c in fb)
    assert any(c.w_off == 1 and c.xs % 4 == 0 and c.x_off == 0 for c in fb)
    assert {c.B for c in fb} == {1, 5} and {c.O for c in fb} == {1, 17}
    # the ranges the ladder gives the named reduction lengths, each worst case below 2^24
    assert [S.linear_ranges(k) for k in (16, 112, 384, 768)] == [(8191, 127), (8191, 16), (1023, 32), (1023, 16)]
    for k in (1, 16, 20, 32, 70, 96, 112, 384, 768):
        a, b = S.linear_ranges(k)
        assert k * a * b + S.BIAS_TOP < 2 ** 24


@pytest.mark.parametrize("case", LINEAR, ids=[c.id for c in LINEAR])
def test_linear_case_and_its_defect_models(case):
    c = case
    # the preconditions, stated again from the case's tensors
    for t in (c.x, c.w) + ((c.b,) if c.b is not None else ()):
        assert E.is_f32(t) and torch.equal(t, t.round())
    bias = c.b.abs() if c.b is not None else 0.0
    assert (c.x.abs() @ c.w.abs().T + bias).max().item() < 2 ** 24
    big = c.x if c.wide == "x" else c.w
    assert S.wide_share(big, 8) >= 0.25 and (c.K > 112 or S.wide_share(big, 11) >= 0.25)
    assert len(torch.unique(c.x, dim=0)) == c.B and len(torch.unique(c.w, dim=0)) == c.O
    assert torch.equal(c.want.double(), c.v) and c.want.dtype == torch.float32
    assert torch.isnan(c.x_full[:, c.K:]).all() and torch.equal(c.x_full[:, :c.K], c.x)
    # the fp32 chain is exact in more than one order: forward, backward and in the lane-strided order of the fallback
    xf, wf = c.x.float(), c.w.float()
    for order in (range(c.K), range(c.K - 1, -1, -1)):
        acc = torch.zeros(c.B, c.O)
        for k in order:
            acc = acc + xf[:, k:k + 1] * wf[:, k].view(1, -1)
        assert torch.equal((acc + (c.b.float() if c.b is not None else 0.0)).double(), c.v)
    for kind in S.LINEAR_MUTANTS:
        m = S.linear_mutant(c, kind)
        if m is not None:
            assert m.shape == c.v.shape and not torch.equal(m, c.v), kind


def test_every_linear_defect_model_shows_somewhere():
    seen = {k: sum(S.linear_mutant(c, k) is not None for c in LINEAR) for k in S.LINEAR_MUTANTS}
    assert all(n > 0 for n in seen.values()), seen
    # the trip faults with every NBT that makes a second trip, the unroll remainder at 1 and 7 steps, the bf16 path everywhere
    assert any(S.linear_mutant(c, "trip2_row") is not None and c.B == 259 for c in LINEAR)
    assert {c.K for c in LINEAR if S.linear_mutant(c, "k_tail6") is not None} >= {16, 112}
    assert seen["bf16_operand"] == len(LINEAR)
    # the mirrored cases: the wide operand on either side, with either path
    assert {(c.mfma, c.wide) for c in LINEAR} == {(True, "x"), (True, "w"), (False, "x"), (False, "w")}


def test_significant_bits():
    v = torch.tensor([0.0, 1.0, 2.0, 3.0, 255.0, 256.0, 257.0, -4097.0, 4096.0, 8191.0, 6144.0], dtype=torch.float64)
    assert S.sig_bits(v).tolist() == [0, 1, 1, 2, 8, 1, 9, 13, 1, 13, 2]
    # what the module docstring says of the ranges: +-2^11 has nothing above 11 bits, +-4096 just under a quarter, +-8191 a half
    full = lambda top: torch.arange(-top, top + 1, dtype=torch.float64)                                   # noqa: E731
    assert S.wide_share(full(2048), 11) == 0.0 and 0.2499 < S.wide_share(full(4096), 11) < 0.25 and S.wide_share(full(8191), 11) > 0.49
    # and a bf16 / fp16 rounding changes exactly the elements counted
    for bits, dt in ((8, torch.bfloat16), (11, torch.float16)):
        t = full(8191)
        assert torch.equal(t.float().to(dt).double() != t, S.sig_bits(t) > bits)


# ------------------------------------------------------------------------------------------------ activations
def test_activation_restatements():
    """gelu_fast_f32 is within the documented 1.5e-7 |v| / 2 (+ fp32 roundings) of the exact-erf GELU, and silu_f32 of the float64 SiLU."""
    x = S.act_input(S.ACT_N[-1])
    assert x.abs().max() > 9 and (x.abs() < 1e-3).any()
    g = (S.gelu_fast_f32(x).double() - S.act_f64(x, "gelu")).abs()
    assert g.max().item() < 4e-7 and g.max().item() > 0
    assert 0 < rel_err(S.silu_f32(x), S.act_f64(x, "silu")) < 1e-6
    assert torch.equal(S.act_f32(x, "none"), x)
    for n in S.ACT_N:
        assert S.act_input(n).shape == (n,)
    assert S.ACT_N[-1] > 2048 * 256                 # a second pass of ds_activation's capped grid


# ------------------------------------------------------------------------------------------------ ds_lstm_layer
LSTM = [S.lstm_case(*s) for s in S.LSTM_SHAPES]


@pytest.mark.parametrize("case", LSTM, ids=["H%d_B%d_T%d" % s for s in S.LSTM_SHAPES])
def test_lstm_defect_models_move_the_result_ten_allowances(case):
    import timbre_ref as R
    c = case
    hs64, last64 = R.lstm_layer(c.pre.double(), c.w_hh)
    hs32, _ = R.lstm_layer(c.pre, c.w_hh)
    assert torch.equal(last64, hs64[:, -1])
    allow = 4 * rel_err(hs32, hs64)
    assert allow > 0
    seen = 0
    for kind in S.LSTM_MUTANTS:
        m = S.lstm_mutant(c, kind)
        if m is None:
            continue
        seen += 1
        moved = rel_err(m, hs64)
        assert moved >= 10 * allow, (kind, moved, allow)
    assert seen >= (1 if c.T == 1 else 2)


def test_lstm_shapes_reach_every_loop_form():
    assert set(S.LSTM_SHAPES) == {(16, 1, 3), (16, 17, 2), (128, 16, 3), (144, 17, 3), (272, 33, 3), (144, 1, 1)}
    hs = {h for h, _, _ in S.LSTM_SHAPES}
    assert any(h < 128 for h in hs) and any(h % 128 == 0 for h in hs) and any(h > 128 and h % 128 for h in hs) and any(h >= 256 for h in hs)
    for kind in S.LSTM_MUTANTS:
        assert any(S.lstm_mutant(c, kind) is not None for c in LSTM), kind


# ------------------------------------------------------------------------------------------------ layout converters
def _layout_shapes():
    for C, Cp in S.LAYOUT_CP:
        for H, W in S.LAYOUT_HW:
            for B in S.LAYOUT_B:
                yield B, C, Cp, H, W


def test_layout_cases_and_defect_models():
    seen = dict.fromkeys(S.LAYOUT_MUTANTS, 0)
    rounds = 0
    for B, C, Cp, H, W in _layout_shapes():
        x = S.layout_input(B, C, H, W)
        assert E.is_f32(x)
        rounds += S.layout_rounds(x)
        for bf16 in (False, True):
            want = S.nhwc_expect(x, Cp, bf16)
            assert want.shape == (B, H, W, Cp) and (want[..., C:] == 0).all()
            assert torch.equal(want[..., :C].double(), E.store(x, bf16).double().permute(0, 2, 3, 1))
            for kind in S.LAYOUT_MUTANTS:
                m = S.nhwc_mutant(x, Cp, bf16, kind, S.NAN)
                if m is not None and not (kind == "bf16_trunc" and not S.layout_rounds(x)):
                    seen[kind] += 1
                    assert not torch.equal(m, want), (kind, B, C, Cp, H, W, bf16)
            for Cs in (C, C + 8):
                src = S.nhwc_source(x, Cs, bf16)
                back = S.nchw_expect(src, C)
                assert torch.equal(back.double(), E.store(x, bf16).double())
                m = S.nchw_mutant(src, C, "cp_as_c", S.NAN)
                assert (m is None) == (Cs == C)
                if m is not None and B * H * W > 1:
                    assert not torch.equal(m, back)
    assert rounds >= 18                                 # every shape of 256 elements or more rounds, with ties (layout_input asserts it)
    assert seen["cp_as_c"] and seen["pads_kept"] and seen["bf16_trunc"]


def test_layout_second_grid_pass():
    """One shape per direction above 8192 x 256 elements; losing the second pass changes the expected tensor."""
    B, C, Cp, H, W = S.LAYOUT_BIG_FWD
    assert S.GRID_ELEMS < B * H * W * Cp <= S.GRID_ELEMS + 4096 and (B, Cp, H * W) == (2, 8, 131200)
    x = S.layout_input(B, C, H, W)
    for bf16 in (False, True):
        want = S.nhwc_expect(x, Cp, bf16)
        m = S.nhwc_mutant(x, Cp, bf16, "pass2_lost", S.NAN)
        assert m is not None and not torch.equal(m, want) and torch.equal(m.flatten()[:S.GRID_ELEMS], want.flatten()[:S.GRID_ELEMS])
    B, C, Cs, H, W = S.LAYOUT_BIG_BACK
    assert S.GRID_ELEMS < B * C * H * W <= S.GRID_ELEMS + 4096
    src = S.nhwc_source(S.layout_input(B, C, H, W), Cs, True)
    want = S.nchw_expect(src, C)
    for kind in ("pass2_lost", "cp_as_c"):
        m = S.nchw_mutant(src, C, kind, S.NAN)
        assert m is not None and not torch.equal(m, want), kind


# ------------------------------------------------------------------------------------------------ ds_dup_batch
def test_dup_batch_cases_and_defect_model():
    assert S.DUP_NBYTES == (16, 4112, 20, 64 * 1024 * 1024 + 48)
    assert S.DUP_NBYTES[3] // 16 > 16384 * 256          # more 16-byte pieces than one pass of the vector kernel's grid
    for n in S.DUP_NBYTES[:3]:
        w = S.dup_words(n)
        assert w.numel() * 4 == n and (w != 0x7FC00000).all()
        assert len(torch.unique(w)) == w.numel()
        want = S.dup_expect(w)
        assert torch.equal(want[:w.numel()], w) and torch.equal(want[w.numel():], w)
        before = torch.full((2 * w.numel(),), 0x7FC00000, dtype=torch.int32)
        assert not torch.equal(S.dup_mutant_second_from_dst0(w, before), want)
    assert [S.dup_path(n, 0, False) for n in S.DUP_NBYTES] == ["vector", "vector", "memcpy", "vector"]
    assert [S.dup_path(n, 0, True) for n in S.DUP_NBYTES] == ["vector_inplace", "vector_inplace", "memcpy", "vector_inplace"]
    assert {S.dup_path(n, 4, False) for n in S.DUP_NBYTES} == {"memcpy"}


# ------------------------------------------------------------------------------------------------ ds_add_layernorm
def test_layernorm_cases():
    ratios = []
    for B in S.LN_B:
        for D in S.LN_D:
            c = S.layernorm_case(B, D)
            assert c.a.shape == c.r.shape == (B, D) and c.a.dtype == torch.float32
            f64, f32 = S.layernorm_ref(c, torch.float64), S.layernorm_ref(c, torch.float32)
            assert torch.isfinite(f64).all() and f32.dtype == torch.float32
            if D > 1:
                # the two-pass formula is torch's layer norm of the summed rows
                want = torch.nn.functional.layer_norm(c.a.double() + c.r.double(), (D,), c.gamma.double(), c.beta.double(), S.LN_EPS)
                assert rel_err(f64, want) < 1e-12
                ratios += S.layernorm_row_ratio(c).tolist()
            else:
                assert torch.equal(f64, c.beta.double().expand(B, 1)) and torch.equal(f32, c.beta.expand(B, 1))
    assert min(ratios) < 0.2 and max(ratios) > 500      # |mean| / std from about 0 to about 1e3


# ------------------------------------------------------------------------------------------------ slabs
def test_slab_on_the_cpu():
    for dt in (torch.float32, torch.bfloat16, torch.int32):
        for off in (0, 1):
            t = torch.arange(10).to(dt).view(2, 5)
            v = S.slab(t, offset_floats=off, device="cpu")
            assert torch.equal(v, t) and v.data_ptr() % 16 == 4 * off
            buf = v.slab_guard[0]
            assert buf.numel() > t.numel() + 64
            if dt != torch.int32:
                assert torch.isnan(buf[:64].float()).all() and torch.isnan(buf[-64:].float()).all()
            S.check_guards(v)
            v.fill_(3)
            S.check_guards(v)                                 # writes inside the view are the kernel's business
            buf[v.slab_guard[1] // t.element_size() - 1] = 0   # the word just in front
            with pytest.raises(AssertionError, match="in front"):
                S.check_guards(v)
            v2 = S.nan_slab((3, 4), dt, device="cpu")
            v2.slab_guard[0][-1] = 0
            with pytest.raises(AssertionError, match="behind"):
                S.check_guards(v2)
