"""The timbre encoder on the GPU: ds_lstm_layer, TimbreEncoder, multi_modal_model and rank_by_prompt against the float64 restatement of
tests/timbre_ref.py and against the reference's own outputs (tests/golden/timbre.npz).

No tolerance here is a constant.  Each comparison measures, in the same run, how far the fp32 CPU restatement lands from the float64 one
(conftest.rel_err: the larger of the max-norm and the rms-relative error) and allows the device four times that distance - the rule of
tests/test_hip_solver.py: a different but fixed fp32 summation order lands a few ulps to either side, not a decade away.  Against the golden
(an fp32 run itself) the device gets the same allowance on top of the golden's own distance to float64."""
import pytest
import torch

import timbre_ref as R
from conftest import rel_err
from diffusynth_amd import _lib as L
from diffusynth_amd.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu


def _check(what, dev, f32, f64, gold=None):
    """dev within 4 x (fp32 CPU restatement vs float64) of float64; and of the golden, on top of the golden's own distance."""
    cpu, err = rel_err(f32, f64), rel_err(dev.cpu(), f64)
    print(f"[timbre] {what}: device vs float64 {err:.3e}, fp32 CPU restatement vs float64 {cpu:.3e}")
    assert tuple(dev.shape) == tuple(f64.shape), what
    assert cpu > 0 and err <= 4 * cpu, (what, err, cpu)
    if gold is not None:
        g64, eg = rel_err(gold, f64), rel_err(dev.cpu(), gold)
        print(f"[timbre] {what}: device vs golden {eg:.3e}, golden vs float64 {g64:.3e}")
        assert eg <= g64 + 4 * cpu, (what, eg, g64, cpu)
    return err, cpu


@pytest.fixture(scope="module")
def golden():
    return R.golden()


def _encoder(case, cfg):
    from diffusynth_amd.timbre import TimbreEncoder
    sd = synth_state_dict(R.keys(case))
    enc = TimbreEncoder(**cfg)
    enc.load_state_dict(sd)
    return sd, enc.cuda()


@pytest.fixture(scope="module")
def small():
    return _encoder("small", R.SMALL_CONFIG)


@pytest.fixture(scope="module")
def prod():
    return _encoder("prod", R.PROD_CONFIG)


# ------------------------------------------------------------------------------------------------ the kernel
def _lstm_layer(pre, w_hh, want_hs=True):
    B, T, H4 = pre.shape
    H = H4 // 4
    ws = torch.full((L.load().ds_lstm_ws_floats(B, H),), float("nan"), device="cuda")      # the workspace need not be initialised
    hs = torch.full((B, T, H), float("nan"), device="cuda") if want_hs else None
    h_last = torch.full((B, H), float("nan"), device="cuda")
    L.call("ds_lstm_layer", pre.data_ptr(), T * H4, H4, w_hh.data_ptr(), B, T, H, L.ptr(hs), h_last.data_ptr(), ws.data_ptr(), L.current_stream())
    return hs, h_last


@pytest.mark.parametrize("B", [1, 3, 17])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_lstm_layer_matches_the_float64_gate_loop(B, T):
    """H = 48: three 16-unit slices, no power of two; B = 17 crosses a 16-sample tile; T = 1 never reads h_prev, T = 2 reads it once."""
    H = 48
    pre = synth_input(f"lstm_pre:{B}:{T}", (B, T, 4 * H))
    w_hh = synth_input("lstm_whh", (4 * H, H), scale=H ** -0.5)
    hs64, last64 = R.lstm_layer(pre.double(), w_hh)
    hs32, last32 = R.lstm_layer(pre, w_hh)
    hs, h_last = _lstm_layer(pre.cuda(), w_hh.cuda())
    _check(f"ds_lstm_layer B={B} T={T} hs", hs, hs32, hs64)
    _check(f"ds_lstm_layer B={B} T={T} h_last", h_last, last32, last64)
    assert torch.equal(h_last, hs[:, -1])
    if (B, T) == (17, 9):                                  # the top layer's form: no hidden sequence wanted
        none, h_last2 = _lstm_layer(pre.cuda(), w_hh.cuda(), want_hs=False)
        assert none is None and torch.equal(h_last2, h_last)


def test_lstm_layer_takes_a_strided_pre():
    """pre as a column block of a wider matrix (batch and step strides above 4H)."""
    B, T, H = 3, 5, 48
    wide = synth_input("lstm_pre_wide", (B, T + 1, 4 * H + 16))
    pre = wide[:, :T, 16:]
    hs64, _ = R.lstm_layer(pre.double(), synth_input("lstm_whh", (4 * H, H), scale=H ** -0.5))
    hs32, _ = R.lstm_layer(pre.contiguous(), synth_input("lstm_whh", (4 * H, H), scale=H ** -0.5))
    d, w = wide.cuda(), synth_input("lstm_whh", (4 * H, H), scale=H ** -0.5).cuda()
    ws = torch.empty(L.load().ds_lstm_ws_floats(B, H), device="cuda")
    hs, h_last = torch.empty(B, T, H, device="cuda"), torch.empty(B, H, device="cuda")
    L.call("ds_lstm_layer", d.data_ptr() + 16 * 4, d.stride(0), d.stride(1), w.data_ptr(), B, T, H, hs.data_ptr(), h_last.data_ptr(), ws.data_ptr(),
           L.current_stream())
    _check("ds_lstm_layer strided pre", hs, hs32, hs64)


def test_timbre_heads_kernel():
    """Ranges that are shorter and longer than a block, rows with a stride."""
    n, stride, B = (300, 5, 64, 270), 650, 3
    z = synth_input("timbre_heads", (B, stride), scale=3.0)
    want64 = [torch.log_softmax(p.double(), 1) if i < 3 else torch.sigmoid(p.double()) for i, p in enumerate(z[:, :sum(n)].split(n, 1))]
    want32 = [torch.log_softmax(p, 1) if i < 3 else torch.sigmoid(p) for i, p in enumerate(z[:, :sum(n)].split(n, 1))]
    d = z.cuda()
    L.call("ds_timbre_heads", d.data_ptr(), stride, B, n[0], n[1], n[2], n[3], L.current_stream())
    assert torch.equal(d[:, sum(n):].cpu(), z[:, sum(n):])                 # columns behind the four ranges are not touched
    for i, p in enumerate(d[:, :sum(n)].split(n, 1)):
        _check(f"ds_timbre_heads range {i}", p, want32[i], want64[i])


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("T", R.SMALL_T)
def test_small_encoder_all_outputs(small, golden, T):
    sd, enc = small
    x = R.small_input(T)
    f64, f32 = R.timbre_encoder(sd, x), R.timbre_encoder(sd, x, torch.float32)
    got = enc(x.cuda())
    assert len(got) == 5
    for k, name in enumerate(R.OUTPUTS):
        _check(f"small T={T} {name}", got[k], f32[k], f64[k], golden[f"small.t{T}.{name}"])
    assert torch.equal(enc.features(x.cuda()), got[0])


@pytest.mark.parametrize("W", R.PROD_W)
def test_production_encoder_all_outputs(prod, golden, W):
    sd, enc = prod
    x = R.prod_input(W)
    f64, f32 = R.timbre_encoder(sd, x), R.timbre_encoder(sd, x, torch.float32)
    got = enc(x.cuda())
    for k, name in enumerate(R.OUTPUTS):
        _check(f"prod W={W} {name}", got[k], f32[k], f64[k], golden[f"prod.w{W}.{name}"])


def test_multi_modal_model_scores_and_ranking(golden):
    from diffusynth_amd.timbre import TimbreEncoder, multi_modal_model, rank_by_prompt
    sd = synth_state_dict(R.keys("mmm"))
    m = multi_modal_model(TimbreEncoder(**R.PROD_CONFIG), None, **R.MMM_CONFIG)
    m.load_state_dict(sd)
    m.cuda()
    x, text, temp = R.prod_input(R.MMM_W), R.text_input(), R.MMM_CONFIG["temperature"]
    f64, f32 = R.mmm(sd, x, text, temp), R.mmm(sd, x, text, temp, torch.float32)
    timbre_emb = m.get_timbre_features(x.cuda())
    text_emb = m.project_text_features(text.cuda())
    scores = m.prompt_scores(text_emb, x.cuda())
    _check("mmm timbre_emb", timbre_emb, f32[0], f64[0], golden["mmm.timbre_emb"])
    _check("mmm text_emb", text_emb, f32[1], f64[1], golden["mmm.text_emb"])
    _check("mmm logits", scores, f32[2], f64[2], golden["mmm.logits"])
    for r in range(2):
        order, s = rank_by_prompt(m, text_emb[r], x.cuda())
        assert order.is_cuda and torch.equal(s, scores[r])
        assert order.tolist() == torch.from_numpy(golden["mmm.logits"][r]).argsort(descending=True).tolist()


def test_a_sample_does_not_depend_on_its_batch(small):
    _, enc = small
    x = R.small_input(9).cuda()
    whole = enc.features(x)
    for i in (0, 16):
        assert torch.equal(whole[i], enc.features(x[i:i + 1])[0]), i


def test_shapes_that_are_not_taken(small):
    _, enc = small
    with pytest.raises(ValueError, match="a \\* b == 32"):
        enc(torch.zeros(2, 4, 9, 5, device="cuda"))
    with pytest.raises(ValueError):
        enc.features(torch.zeros(2, 32, 5, device="cuda"))
    H = 40
    pre, w = torch.zeros(2, 3, 4 * H, device="cuda"), torch.zeros(4 * H, H, device="cuda")
    with pytest.raises(L.DsError, match="H=40"):
        _lstm_layer(pre, w)
    # nothing was launched: the outputs keep what they held
    ws = torch.full((L.load().ds_lstm_ws_floats(2, H),), 7.0, device="cuda")
    h_last = torch.full((2, H), 7.0, device="cuda")
    rc = L.load().ds_lstm_layer(pre.data_ptr(), 3 * 4 * H, 4 * H, w.data_ptr(), 2, 3, H, None, h_last.data_ptr(), ws.data_ptr(), L.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((h_last == 7.0).all()) and bool((ws == 7.0).all())


def test_calls_follow_the_callers_stream(prod):
    """Two calls of different lengths back to back on a side stream, nothing synchronised in between: the same bits as on the default stream."""
    _, enc = prod
    xa, xb = R.prod_input(64).cuda(), R.prod_input(20).cuda()
    want_a, want_b = enc.features(xa), enc.features(xb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_a = enc.features(xa)
        got_b = enc.features(xb)
    side.synchronize()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
