"""Plain CPU helpers of tests/test_hip_support_kernels.py and tests/test_support_ref_cpu.py: the fp32 dense and layout kernels of
csrc/misc.hip (ds_linear, ds_activation, ds_add_layernorm, ds_nchw_to_nhwc, ds_nhwc_to_nchw, ds_dup_batch) and the recurrent product of
ds_lstm_layer (csrc/lstm.hip).

Four kinds of thing live here:
  case builders   every input of a GPU test, with the case's preconditions asserted BEFORE anything is launched;
  references      the operation in float64 (exact data: the expected tensor bit for bit, tests/exact_ref.py explains why);
  restatements    the kernel's own formula in torch fp32 on the CPU: the yardstick of the measured tolerance rule (the device may land four
                  times as far from float64 as the restatement does, tests/test_hip_timbre.py);
  defect models   ("mutants") what a kernel with one named indexing or arithmetic fault would produce.  The CPU test shows that each moves
                  the expected tensor, so a kernel with that fault cannot pass the GPU test.

Exact data for ds_linear: integer operands, sum |x||w| + |bias| < 2^24 at every output, so every fp32 partial sum is exact in any order (the
16x16x4 fp32 MFMA and the fallback's fmaf + wave sum are fp32 fma chains) and the stored value IS the float64 value.  The operand ranges
follow the reduction length by the fixed ladder LADDER: the first step whose worst case K * top_wide * top_narrow + BIAS_TOP stays below
2^24; nothing a kernel computes enters the choice.  One operand (the "wide" one) is drawn from a range that needs more significant bits than
a reduced-precision operand path carries: more than 8 (bf16) on at least a quarter of its elements in every case, more than 11 (fp16, tf32)
for K <= 112.  (+-4096 would leave 24.997 % of the integers above 11 bits and +-2^11 none, so the two short steps of the ladder take
+-8191: half of those integers need 12 or 13 bits.)"""
import functools
import types

import torch
import torch.nn.functional as F

import exact_ref as E
from diffusynth_amd.synth import synth_input

NAN = float("nan")


# ================================================================================================= slabs
def slab(tensor, front=64, back=64, offset_floats=0, device="cuda"):
    """`tensor` (fp32, bf16 or int32; any shape) as a view inside a larger allocation on `device` whose every other word is NaN (int32: the
    bit pattern of a NaN): `front` floats in front (a multiple of four), `back` behind, and `offset_floats` more in front, which put the view
    4-byte but not 16-byte aligned when they are no multiple of four.  gn_partials_ref.guarded is the model.  A stray WRITE changes a guard
    word (check_guards), a stray READ that reaches a result shows there as NaN.  This is no proof of memory safety: a read whose value is
    discarded, or that lands inside the view, is not seen.  Returns the view; the allocation rides on it for check_guards."""
    assert front % 4 == 0 and front > 0 and back > 0 and offset_floats >= 0
    per = 4 // tensor.element_size()
    assert per in (1, 2)
    n = tensor.numel()
    lead = (front + offset_floats) * per
    total = lead + n + back * per
    total += (-total) % per
    fill = 0x7FC00000 if tensor.dtype == torch.int32 else NAN
    buf = torch.full((total,), fill, dtype=tensor.dtype, device=device)
    view = buf[lead:lead + n].view(tensor.shape)
    view.copy_(tensor)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * offset_floats) % 16
    raw = buf.view(torch.uint8)
    lo, hi = lead * tensor.element_size(), (lead + n) * tensor.element_size()
    view.slab_guard = (buf, lo, hi, raw[:lo].clone(), raw[hi:].clone())
    return view


def nan_slab(shape, dtype=torch.float32, device="cuda", **kw):
    """An output buffer: a slab whose view is NaN too (int32: NaN bit patterns)."""
    fill = 0x7FC00000 if dtype == torch.int32 else NAN
    return slab(torch.full(tuple(shape), fill, dtype=dtype, device=device), device=device, **kw)


def check_guards(*views):
    """The guard words of these slabs are bit-identical to what slab() wrote."""
    for v in views:
        buf, lo, hi, front, back = v.slab_guard
        raw = buf.view(torch.uint8)
        assert torch.equal(raw[:lo], front), "a write in front of the slab's view"
        assert torch.equal(raw[hi:], back), "a write behind the slab's view"


# ================================================================================================= significant bits
def sig_bits(v):
    """Significant bits of each element of an integer-valued float64 tensor: bit length minus trailing zeros (0 for 0)."""
    n = v.abs().to(torch.int64)
    assert torch.equal(n.double(), v.abs().double()) and int(n.max()) < (1 << 40)
    bitlen = torch.zeros_like(n)
    ctz = torch.zeros_like(n)
    m = n.clone()
    for _ in range(41):
        bitlen += (m > 0)
        m = m >> 1
    m = n.clone()
    live = n > 0
    for _ in range(41):
        step = live & ((m & 1) == 0)
        ctz += step
        live = step
        m = m >> 1
    return bitlen - ctz


def wide_share(v, bits):
    """Share of the elements that need more than `bits` significant bits."""
    return (sig_bits(v) > bits).double().mean().item()


# ================================================================================================= ds_linear, exact data
# (top of the wide operand, top of the narrow one): the first step with K * wide * narrow + BIAS_TOP < 2^24
LADDER = [(8191, 127), (8191, 16), (1023, 32), (1023, 16), (255, 16), (255, 4)]
BIAS_TOP = 255
LINEAR_MUTANTS = ("trip2_row", "k_tail6", "o_clamp_store", "bias_o0", "xs_as_K", "bf16_operand")


def linear_ranges(K):
    for wide, narrow in LADDER:
        if K * wide * narrow + BIAS_TOP < E.LIMIT:
            return wide, narrow
    raise AssertionError("no step of LADDER fits K = %d" % K)


def nbt_of(B):
    """The batch tiles per trip the launcher of ds_linear picks (misc.hip)."""
    return 1 if B <= 16 else 2 if B <= 32 else 4 if B <= 64 else 8


def _seed(*key):
    return sum((i + 1) * 7919 * ord(ch) for i, ch in enumerate(str(key))) % (1 << 31)


def _distinct_rows(g, t, top):
    """Redraw (seeded) every row that repeats an earlier one until all rows differ."""
    for _ in range(64):
        _, inv = torch.unique(t, dim=0, return_inverse=True)
        first = torch.full((int(inv.max()) + 1,), t.shape[0], dtype=torch.long).scatter_reduce(0, inv, torch.arange(t.shape[0]), "amin")
        dup = first[inv] != torch.arange(t.shape[0])
        if not dup.any():
            return t
        t[dup] = E.ints(g, (int(dup.sum()), t.shape[1]), -top, top)
    raise AssertionError("rows do not become distinct: %d rows of %d values in +-%d" % (t.shape[0], t.shape[1], top))


@functools.lru_cache(maxsize=None)
def linear_case(B, K, O, bias=True, xpad=0, ypad=5, wide="x", x_off=0, w_off=0, y_off=0):
    """One exact ds_linear call.  xpad: x is the first K columns of a [B][K + xpad] matrix whose other columns are NaN (xs = K + xpad);
    ypad: y is [B][O + ypad], prefilled with NaN; *_off: the operand starts that many floats past a 16-byte boundary; wide: which operand
    carries the many-bit values.  Fields: x_full [B][xs] and x [B][K], w [O][K], b [O] or None (float64 integers), v = the exact result
    (float64), want = v in fp32, mfma = whether the launcher takes the matrix-core kernel."""
    g = E.gen(_seed("linear", B, K, O, bias, xpad, wide))
    top_w, top_n = linear_ranges(K)
    xt, wt = (top_w, top_n) if wide == "x" else (top_n, top_w)
    x = _distinct_rows(g, E.ints(g, (B, K), -xt, xt), xt)
    w = _distinct_rows(g, E.ints(g, (O, K), -wt, wt), wt)
    b = E.ints(g, (O,), -BIAS_TOP, BIAS_TOP) if bias else None
    # ---- preconditions
    assert E.is_f32(x) and E.is_f32(w) and (b is None or E.is_f32(b))
    assert len(torch.unique(x, dim=0)) == B and len(torch.unique(w, dim=0)) == O
    margin = (x.abs() @ w.abs().T + (b.abs() if bias else 0.0)).max().item()
    E.check_exact(margin)
    big = x if wide == "x" else w
    assert wide_share(big, 8) >= 0.25, "only %.3f of the wide operand need more than 8 bits" % wide_share(big, 8)
    if K <= 112:
        assert wide_share(big, 11) >= 0.25, "only %.3f of the wide operand need more than 11 bits" % wide_share(big, 11)
    v = x @ w.T + (b if bias else 0.0)
    assert E.is_f32(v)
    x_full = torch.full((B, K + xpad), NAN, dtype=torch.float64)
    x_full[:, :K] = x
    xs = K + xpad
    mfma = K % 16 == 0 and xs % 4 == 0 and x_off % 4 == 0 and w_off % 4 == 0
    return types.SimpleNamespace(id="B%d_K%d_O%d%s%s_wide%s%s%s%s" % (B, K, O, "" if bias else "_nobias", "_xs+%d" % xpad if xpad else "", wide,
                                                                      "_xoff" if x_off else "", "_woff" if w_off else "", "_yoff" if y_off else ""),
                                 B=B, K=K, O=O, xs=xs, ys=O + ypad, x=x, x_full=x_full, w=w, b=b, v=v, want=E.store(v, False), margin=margin,
                                 wide=wide, x_off=x_off, w_off=w_off, y_off=y_off, mfma=mfma, nbt=nbt_of(B) if mfma else 0)


def linear_mutant(c, kind):
    """The float64 result of a ds_linear with one fault, or None where the fault cannot show in this case.
    trip2_row      rows of the second and later bt0 trips (b >= 16 NBT) all computed from row B - 1 of x;
    k_tail6        the 16-deep K steps behind the last multiple of 6 dropped (a lost remainder of `#pragma unroll 6`);
    o_clamp_store  the store's column clamped to O - 1 like the load's: the lanes of the ragged tile write their bias-free sums there;
    bias_o0        the bias of a tile's first column used for all 16;
    xs_as_K        row b of x read at b * K instead of b * xs;
    bf16_operand   the wide operand rounded to bf16 on its way into the matrix cores."""
    x, w, b = c.x, c.w, c.b
    bias = b if b is not None else torch.zeros(c.O, dtype=torch.float64)
    if kind == "trip2_row":
        if not c.mfma or c.B - 1 <= 16 * c.nbt:                 # (B - 1 == 16 NBT: the one row of the second trip IS row B - 1)
            return None
        x2 = x.clone()
        x2[16 * c.nbt:] = x[c.B - 1]
        return x2 @ w.T + bias
    if kind == "k_tail6":
        steps = c.K // 16
        if not c.mfma or steps % 6 == 0:
            return None
        keep = steps // 6 * 6 * 16
        return x[:, :keep] @ w[:, :keep].T + bias
    if kind == "o_clamp_store":
        if not c.mfma or c.O % 16 == 0 or b is None or b[c.O - 1] == 0:
            return None
        v = c.v.clone()
        v[:, c.O - 1] -= b[c.O - 1]
        return v
    if kind == "bias_o0":
        if b is None or c.O == 1:
            return None
        return x @ w.T + b[torch.arange(c.O) // 16 * 16]
    if kind == "xs_as_K":
        if c.xs == c.K or c.B == 1:
            return None
        flat = c.x_full.flatten()
        x2 = torch.stack([flat[i * c.K:(i + 1) * c.K] for i in range(c.B)])
        return x2 @ w.T + bias
    if kind == "bf16_operand":
        r = lambda t: t.float().bfloat16().double()                                                       # noqa: E731
        return (r(x) @ w.T if c.wide == "x" else x @ r(w).T) + bias
    raise ValueError(kind)


LIN_B = {1: (1, 16), 2: (17, 32), 4: (33, 64), 8: (65, 128, 129)}
LIN_O = (1, 15, 16, 17, 64, 65)
LIN_K = (16, 96, 112, 384)


def linear_mfma_args():
    """The covering set of the matrix-core path: with every NBT every O and every K (and every B of that NBT), the variants bias = NULL,
    xs = K + 16 and y one float off a 16-byte boundary each with every NBT, the wide operand alternating sides; ys = O + 5 throughout.
    Then B = 259 (a ragged third trip) at K = 112, O = 65, plain and as a column block, and K = 768, O = 48, B = 40."""
    out = []
    for nbt, bs in LIN_B.items():
        for i, O in enumerate(LIN_O):
            B, K = bs[i % len(bs)], LIN_K[(i + nbt) % 4]
            out.append(dict(B=B, K=K, O=O, bias=i % 3 != 0, xpad=16 if i % 3 == 1 else 0, y_off=1 if i % 3 == 2 else 0, wide="xw"[i % 2]))
    out.append(dict(B=259, K=112, O=65))
    out.append(dict(B=259, K=112, O=65, xpad=16, wide="w", y_off=1))
    out.append(dict(B=40, K=768, O=48))
    return out


def linear_fallback_args():
    """The one-wave-per-output kernel, reached by each of its four conditions (K % 16, xs % 4, x alignment, W alignment), at B in {1, 5}
    and O in {1, 17}."""
    out = []
    out.append(dict(B=5, K=1, O=17, wide="w"))
    out.append(dict(B=1, K=20, O=1, bias=False))
    out.append(dict(B=5, K=70, O=17, wide="w"))
    out.append(dict(B=1, K=70, O=1))
    out.append(dict(B=5, K=32, O=17, xpad=1))
    out.append(dict(B=1, K=32, O=1, xpad=1, wide="w"))
    out.append(dict(B=5, K=32, O=1, x_off=1))
    out.append(dict(B=1, K=32, O=17, x_off=1, bias=False, wide="w"))
    out.append(dict(B=5, K=32, O=17, w_off=1, wide="w"))
    out.append(dict(B=1, K=32, O=1, w_off=1, xpad=16))
    return out


def linear_cases():
    return [linear_case(**a) for a in linear_mfma_args() + linear_fallback_args()]


# ================================================================================================= activations (fp32 restatements)
def _f32(t):
    return t.float().double()


def gelu_fast_f32(x):
    """gelu_fast of csrc/common.hpp, step by step with ONE fp32 rounding per operation (products and fused multiply-adds are formed in float64,
    where 24 x 24 bits are exact): relu(v) - 0.5 |v| q, q = poly(t) t exp(-v^2 / 2), t = 1 / (1 + 0.3275911 |v| / sqrt 2) (Abramowitz & Stegun
    7.1.26).  The device's v_rcp_f32 and v_exp_f32 are within an ulp of the correctly rounded values used here."""
    c = lambda s: _f32(torch.tensor(s, dtype=torch.float64))                                              # noqa: E731
    fma = lambda p, q, r: _f32(p * q + r)                                                                 # noqa: E731
    v = x.float().double()
    av = v.abs()
    t = _f32(1.0 / fma(c(0.3275911 * 0.70710678118654752440), av, 1.0))
    poly = fma(c(1.061405429), t, c(-1.453152027))
    for k in (1.421413741, -0.284496736, 0.254829592):
        poly = fma(poly, t, c(k))
    e = _f32(torch.exp2(_f32(_f32(v * v) * c(-0.5 * 1.44269504088896340736))))
    return fma(-0.5 * av, _f32(_f32(poly * t) * e), v.clamp_min(0.0)).float()


def silu_f32(x):
    """act_apply's SiLU: v / (1 + expf(-v)) in fp32."""
    x = x.float()
    return x / (1.0 + torch.exp(-x))


def act_f32(x, act):
    return {"none": lambda v: v.float(), "gelu": gelu_fast_f32, "silu": silu_f32}[act](x)


def act_f64(x, act):
    x = x.double()
    return {"none": lambda v: v, "gelu": E.gelu64, "silu": lambda v: v * torch.sigmoid(v)}[act](x)


ACT_N = (1, 255, 257, 2048 * 256 + 3)          # one element, under and over a block, a second pass of the 2048-block grid


@functools.lru_cache(maxsize=None)
def act_input(n):
    """N(0, 3^2) inputs: both tails of the two activations and the steep part around zero."""
    return synth_input("support_act:%d" % n, (n,), 3.0)


@functools.lru_cache(maxsize=None)
def linear_random_case(B, K, O):
    return types.SimpleNamespace(x=synth_input("support_lin_x:%d:%d" % (B, K), (B, K)), w=synth_input("support_lin_w:%d:%d" % (O, K), (O, K), K ** -0.5),
                                 b=synth_input("support_lin_b:%d" % O, (O,)), B=B, K=K, O=O)


def linear_act_refs(c, act):
    """(fp32 restatement, float64) of ds_linear with act_in on a random case."""
    return F.linear(act_f32(c.x, act), c.w, c.b), F.linear(act_f64(c.x, act), c.w.double(), c.b.double())


# ================================================================================================= ds_lstm_layer
# H = 16: one 16-deep step and nothing else; 128: one 128-deep trip, no tail; 144: a trip and a one-step tail; 272: two trips and a tail.
# B = 1, 16 (a full tile), 17 and 33 (ragged second and third tile); T = 1 never reads h, T = 2 reads it once, T = 3 through both buffers.
LSTM_SHAPES = ((16, 1, 3), (16, 17, 2), (128, 16, 3), (144, 17, 3), (272, 33, 3), (144, 1, 1))
LSTM_MUTANTS = ("tail_dropped", "acc3_lost", "gates_permuted")


@functools.lru_cache(maxsize=None)
def lstm_case(H, B, T):
    return types.SimpleNamespace(H=H, B=B, T=T, pre=synth_input("support_lstm_pre:%d:%d:%d" % (H, B, T), (B, T, 4 * H)),
                                 w_hh=synth_input("support_lstm_whh:%d" % H, (4 * H, H), H ** -0.5))


def lstm_mutant(c, kind):
    """hs (float64) of an LSTM layer with one fault in the recurrent product, or None where it cannot show.
    tail_dropped    the 16-deep steps behind the last 128-deep trip not summed (all of them where H < 128);
    acc3_lost       the last of the four accumulator chains (steps 3 and 7 of every trip) left out of the final sum;
    gates_permuted  the gate rows taken in the order i, g, f, o."""
    H, B, T = c.H, c.B, c.T
    pre, w = c.pre.double(), c.w_hh.double().clone()
    keep = torch.ones(H, dtype=torch.float64)
    order = (0, 1, 2, 3)
    if kind == "tail_dropped":
        if T == 1 or H % 128 == 0:
            return None
        keep[H // 128 * 128:] = 0
    elif kind == "acc3_lost":
        if T == 1 or H < 128:
            return None
        k = torch.arange(H)
        keep[(k < H // 128 * 128) & ((k % 128) // 16 % 4 == 3)] = 0
    elif kind == "gates_permuted":
        order = (0, 2, 1, 3)
    else:
        raise ValueError(kind)
    w = w * keep
    h = cst = torch.zeros(B, H, dtype=torch.float64)
    hs = []
    for t in range(T):
        z = pre[:, t] + h @ w.T if t else pre[:, t]
        parts = z.split(H, dim=1)
        i, f, g, o = (parts[j] for j in order)
        cst = torch.sigmoid(f) * cst + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(cst)
        hs.append(h)
    return torch.stack(hs, 1)


# ================================================================================================= layout converters
GRID_ELEMS = 8192 * 256                        # blocks_for's cap: the grid-stride loops make a second pass above this many elements
LAYOUT_CP = ((4, 4), (4, 8), (3, 8), (80, 80))
LAYOUT_HW = ((1, 1), (5, 3), (37, 9))
LAYOUT_B = (1, 3)
LAYOUT_BIG_FWD = (2, 3, 8, 400, 328)           # B, C, Cp, H, W: 2 x 131,200 x 8 elements, 2,048 more than one pass
LAYOUT_BIG_BACK = (2, 8, 16, 400, 328)         # B, C, Cs, H, W
LAYOUT_MUTANTS = ("cp_as_c", "pads_kept", "bf16_trunc", "pass2_lost")


@functools.lru_cache(maxsize=None)
def layout_input(B, C, H, W):
    """NCHW integers / 16 of +-2047: exact in fp32, more than 8 significant bits on most, 9-bit values (exact bf16 ties) among them."""
    x = E.ints(E.gen(_seed("layout", B, C, H, W)), (B, C, H, W), -2047, 2047, scale=1.0 / 16)
    assert E.is_f32(x)
    if x.numel() >= 256:
        E.check_rounding(x)
    return x


def layout_rounds(x):
    share, ties = E.rounding_profile(x)
    return share >= 0.005 and ties > 0


def nhwc_expect(x, Cp, bf16):
    """What ds_nchw_to_nhwc stores: [B][H][W][Cp], one rounding to the output type, pad channels exact zeros."""
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, Cp, dtype=torch.bfloat16 if bf16 else torch.float32)
    out[..., :C] = E.store(x.permute(0, 2, 3, 1), bf16)
    return out


def nhwc_source(x, Cs, bf16):
    """An NHWC source of ds_nhwc_to_nchw with channel stride Cs: the values of x (bf16: rounded once) in the first C channels, NaN behind."""
    B, C, H, W = x.shape
    src = torch.full((B, H, W, Cs), NAN, dtype=torch.bfloat16 if bf16 else torch.float32)
    src[..., :C] = E.store(x.permute(0, 2, 3, 1), bf16)
    return src


def nchw_expect(src, C):
    """What ds_nhwc_to_nchw stores for that source: fp32 NCHW, a copy of the stored values."""
    return src[..., :C].float().permute(0, 3, 1, 2).contiguous()


def nhwc_mutant(x, Cp, bf16, kind, prefill):
    """ds_nchw_to_nhwc with one fault (a tensor like nhwc_expect's, over a buffer prefilled with `prefill`), or None where it cannot show.
    cp_as_c: the element index decomposed with C instead of Cp; pads_kept: pad channels not written; bf16_trunc: the bf16 store truncates;
    pass2_lost: elements behind the first grid pass not written."""
    B, C, H, W = x.shape
    want = nhwc_expect(x, Cp, bf16)
    if kind == "cp_as_c":
        if Cp == C:
            return None
        flat = torch.full((want.numel(),), prefill, dtype=want.dtype)
        flat[:B * H * W * C] = want[..., :C].flatten()
        return flat.view(want.shape)
    if kind == "pads_kept":
        if Cp == C:
            return None
        want[..., C:] = prefill
        return want
    if kind == "bf16_trunc":
        if not bf16:
            return None
        want[..., :C] = E.trunc_bf16(x.permute(0, 2, 3, 1))
        return want
    if kind == "pass2_lost":
        if want.numel() <= GRID_ELEMS:
            return None
        flat = want.flatten().clone()
        flat[GRID_ELEMS:] = prefill
        return flat.view(want.shape)
    raise ValueError(kind)


def nchw_mutant(src, C, kind, prefill):
    """ds_nhwc_to_nchw with one fault: cp_as_c (the source's channel stride taken as C) or pass2_lost; None where it cannot show."""
    B, H, W, Cs = src.shape
    want = nchw_expect(src, C)
    if kind == "cp_as_c":
        if Cs == C:
            return None
        return src.flatten()[:B * H * W * C].view(B, H, W, C).float().permute(0, 3, 1, 2).contiguous()
    if kind == "pass2_lost":
        if want.numel() <= GRID_ELEMS:
            return None
        flat = want.flatten().clone()
        flat[GRID_ELEMS:] = prefill
        return flat.view(want.shape)
    return None


# ================================================================================================= ds_dup_batch
DUP_VEC_PASS = 16384 * 256 * 16                # bytes one pass of the vector kernel's capped grid copies: 64 MiB
DUP_NBYTES = (16, 4096 + 16, 20, DUP_VEC_PASS + 48)


def dup_words(nbytes, device="cpu"):
    """nbytes / 4 int32 words, every one different from its neighbours and from the word 4, 16 or nbytes bytes away (a multiplicative hash of
    the index), none the NaN pattern of the guards."""
    assert nbytes % 4 == 0
    i = torch.arange(nbytes // 4, dtype=torch.int64, device=device)
    return ((i * 2654435761 + 12345) % 2147483629).to(torch.int32)


def dup_expect(words):
    return torch.cat([words, words])


def dup_mutant_second_from_dst0(words, dst_before):
    """The second half copied from offset 0 of dst as it was before the call (a copy that reads dst instead of src): the not-in-place forms
    only, where dst held something else."""
    return torch.cat([words, dst_before[:words.numel()]])


def dup_path(nbytes, src_off_bytes, inplace):
    """Which of ds_dup_batch's three paths a call takes."""
    if nbytes % 16 or src_off_bytes % 16:
        return "memcpy"
    return "vector_inplace" if inplace else "vector"


# ================================================================================================= ds_add_layernorm
LN_B = (1, 5)
LN_D = (1, 37, 256, 257, 512, 1000)            # one element, under / at / over one block stride of 256, two strides, ragged fourth
LN_RATIOS = (0.0, 1.0, 10.0, 100.0, 1000.0)    # |mean| / std of a row of a + r
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def layernorm_case(B, D):
    """a + r = noise of std ~1 plus ratio (rows of B = 5: every ratio; the one row of B = 1: the ratios in turn over D), r a third of it."""
    tag = "support_ln:%d:%d" % (B, D)
    noise = synth_input(tag + ":n", (B, D))
    first = LN_D.index(D) if B == 1 else 0
    ratio = torch.tensor([LN_RATIOS[(first + b) % 5] * (-1) ** b for b in range(B)]).view(B, 1)
    s = noise + ratio
    r = (s / 3 + synth_input(tag + ":r", (B, D), 0.5)).float()
    a = (s - r).float()
    return types.SimpleNamespace(B=B, D=D, a=a, r=r, gamma=1 + 0.2 * synth_input(tag + ":g", (D,)), beta=0.3 * synth_input(tag + ":b", (D,)),
                                 ratio=ratio.flatten())


def layernorm_ref(c, dtype):
    """The kernel's two-pass formula (mean, then the centred second moment, eps inside the square root) in `dtype`: float64 is the yardstick,
    float32 the restatement.  The sum a + r is formed in `dtype` from the fp32 inputs."""
    s = c.a.to(dtype) + c.r.to(dtype)
    mean = s.mean(1, keepdim=True)
    d = s - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + LN_EPS)
    return d * rstd * c.gamma.to(dtype) + c.beta.to(dtype)


def layernorm_row_ratio(c):
    s = c.a.double() + c.r.double()
    return (s.mean(1).abs() / s.std(1, unbiased=False).clamp_min(1e-30)) if c.D > 1 else torch.zeros(c.B, dtype=torch.float64)

