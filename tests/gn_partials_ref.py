"""Float64 restatement of the GroupNorm-from-partials contract and the inputs of tests/test_gn_partials_cpu.py and
tests/test_hip_gn_partials.py (plain numpy / torch on the CPU; only guarded() touches a device).

A producer writes per-block (sum, sumsq) fp32 partials [B][parts][2]; a consumer sums them in float64 and uses
(rstd, rstd * mean) with mean = s1 / count, var = max(s2 / count - mean^2, 0).  The helpers below build partials whose
layout makes every indexing fault loud (first and last chunk a quarter of the sample each, samples of different scale
and offset, NaN around the buffer), and the case builders restate each consumer's operation in float64 as a function of
the statistics, so that the CPU test can show that wrong statistics move the result far beyond the GPU test's tolerance."""
import functools
import types

import torch
import torch.nn.functional as F

from diffusynth_amd.synth import synth_input, synth_state_dict

# per-sample scale and offset (cycled over the batch): |mean| / std = 1.6, 2.3, 1.8, 1.6, 1.8 — far enough from zero that a lost or
# foreign chunk moves mean AND variance by tens of percent, below 3 so that fp32 (sum, sumsq) partials still carry the variance
SCALES = (1.0, 0.35, 2.5, 0.7, 1.7)
OFFSETS = (1.6, -0.8, 4.5, -1.1, 3.0)
EPS = 1e-5
MUTANTS = ("M1", "M2", "M3", "M4", "M5", "M6")


def distinct_samples(tag, shape, gain=1.0):
    """synth_input with a per-sample scale and offset (times ``gain``): no sample's statistics fit another sample."""
    x = synth_input(tag, shape)
    for b in range(shape[0]):
        x[b] = (x[b] * SCALES[b % 5] + OFFSETS[b % 5]) * gain
    return x


def chunk_bounds(n, parts):
    """parts contiguous chunks of n elements: the first and the last hold about a quarter each, the rest is spread evenly
    (chunks may be empty where parts exceeds the elements in between: their partial is (0, 0))."""
    if parts == 1:
        return [0, n]
    if parts == 2:
        return [0, n // 2, n]
    q = max(n // 4, 1)
    inner = torch.linspace(q, n - q, parts - 1, dtype=torch.float64).round().long().tolist()
    return [0] + inner + [n]


def make_partials(x_stored, parts):
    """fp32 [B][parts][2] chunk (sum, sumsq) of each sample's flattened STORED values (bf16-rounded, or hi + lo planes; NHWC order),
    computed in float64 and then rounded."""
    xd = x_stored.double().flatten(1)
    bnd = chunk_bounds(xd.shape[1], parts)
    out = torch.zeros(xd.shape[0], parts, 2, dtype=torch.float64)
    for i in range(parts):
        c = xd[:, bnd[i]:bnd[i + 1]]
        out[:, i, 0] = c.sum(1)
        out[:, i, 1] = (c * c).sum(1)
    return out.float()


def ab_of_sums(s, count, eps=EPS):
    mean = s[..., 0] / count
    var = (s[..., 1] / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return torch.stack([rstd, rstd * mean], -1)


def ab_from_partials(part, count, eps=EPS):
    """The contract: float64 sum of the fp32 partials -> (rstd, rstd * mean) per sample, float64 [B][2]."""
    return ab_of_sums(part.double().sum(1), float(count), eps)


def ab_direct(x_stored, eps=EPS):
    """(rstd, rstd * mean) straight from the stored values in float64 (what hip_helpers.gn_ab_of computes)."""
    xd = x_stored.double().flatten(1)
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps)
    return torch.stack([rstd, rstd * mean], 1)


def order_independent(part, count, eps=EPS):
    """True when the float64 sum of these fp32 partials gives the same fp32 (rstd, rstd * mean) in several summation orders (forward,
    backward, lane-strided as a 64-lane wave or a 256-thread block walks them, pairwise): the premise of bit-identity between a
    kernel's gn_part form and its gn_ab form fed by ds_gn_finalize."""
    p = part.double()
    B, n, _ = p.shape

    def strided(lanes):
        pad = torch.zeros(B, (-n) % lanes, 2, dtype=torch.float64)
        q = torch.cat([p, pad], 1).view(B, -1, lanes, 2)
        acc = torch.zeros(B, lanes, 2, dtype=torch.float64)
        for i in range(q.shape[1]):
            acc = acc + q[:, i]
        while acc.shape[1] > 1:                       # butterfly / tree over the lanes
            h = acc.shape[1] // 2
            acc = acc[:, :h] + acc[:, h:]
        return acc[:, 0]

    def serial(order):
        acc = torch.zeros(B, 2, dtype=torch.float64)
        for i in order:
            acc = acc + p[:, i]
        return acc

    sums = [p.sum(1), serial(range(n)), serial(range(n - 1, -1, -1)), strided(64), strided(256)]
    abs_ = [ab_of_sums(s, float(count), eps).float() for s in sums]
    return all(torch.equal(abs_[0], a) for a in abs_[1:])


def mutant_ab(part, count, kind, eps=EPS):
    """Statistics a faulty reducer would use, float64 [B][2], or None where the fault cannot occur at this number of partials.
    M1: sample b normalised with sample (b + 1) % B's statistics; M2 / M3: partials with index >= 256 / >= 64 dropped; M4: the last
    partial dropped; M5: one partial too many (the next sample's first one); M6: the first partial dropped."""
    p = part.double().clone()
    B, n, _ = p.shape
    if kind == "M1":
        return ab_from_partials(part, count, eps).roll(-1, 0) if B > 1 else None
    if kind == "M2":
        if n <= 256:
            return None
        p[:, 256:] = 0
    elif kind == "M3":
        if n <= 64:
            return None
        p[:, 64:] = 0
    elif kind == "M4":
        if n < 2:
            return None
        p[:, -1] = 0
    elif kind == "M5":
        if B < 2:
            return None
        return ab_of_sums(p.sum(1) + p[:, 0].roll(-1, 0), float(count), eps)
    elif kind == "M6":
        if n < 2:
            return None
        p[:, 0] = 0
    else:
        raise ValueError(kind)
    return ab_of_sums(p.sum(1), float(count), eps)


def guarded(part, device="cuda"):
    """The partials inside a larger device allocation: 6 floats of NaN in front, NaN behind — the base is 8-byte but not 16-byte
    aligned, and a read outside [B][parts][2] meets NaN or the neighbouring (different) sample.  Returns the [B][parts][2] view."""
    n = part.numel()
    buf = torch.full((6 + n + 58,), float("nan"), dtype=torch.float32, device=device)
    view = buf[6:6 + n].view(part.shape)
    view.copy_(part)
    assert view.data_ptr() % 16 == 8
    return view


def gn(x, ab, gamma, beta):
    """GroupNorm(1, C) of NCHW x with GIVEN statistics ab [B][2] = (rstd, rstd * mean), float64."""
    B = x.shape[0]
    a, am = ab[:, 0].view(B, 1, 1, 1), ab[:, 1].view(B, 1, 1, 1)
    return (x.double() * a - am) * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)


def bf16r(t):
    return t.bfloat16().float()


def split_sum(t):
    """What the split-precision kernels see of an fp32 tensor: bf16(x) + bf16(x - bf16(x)) (x to 2^-17)."""
    hi = t.float().bfloat16().float()
    return hi + (t.float() - hi).bfloat16().float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def case_partials(case, parts):
    """Partials of a case's input in the order it is stored on the device (channels-last)."""
    return make_partials(nhwc(case.stored), parts)


# ------------------------------------------------------------------------------------------------ cases
# Every builder returns a namespace with: id, tol (the tolerance of the kernel's existing gn_ab test in tests/test_hip_kernels.py),
# parts (the partial counts the GPU test runs), stored (NCHW fp32: the values the kernel reads), count, ref(ab) -> float64 NCHW
# reference of the consumer's operation for statistics ab, and the raw operands the GPU test uploads.
PARTS = (1, 65, 300)
PARTS_HALO = (1, 64, 65, 256, 257, 300)      # the halo kernel prefetches 4 x 64 pairs and walks the rest: both edges straddled


@functools.lru_cache(maxsize=None)
def gn_apply_case(dt, Cc, HW, B=3, res=True, cbias=False, act="none"):
    """ds_gn_apply with G = 1: act(GN(x)) + cbias + res on the stored values.  dt: "bf16" / "f32"."""
    tag = "gp_ga_%s_%d_%d_%d" % (dt, Cc, HW, B)
    rnd = bf16r if dt == "bf16" else (lambda t: t)
    x = rnd(distinct_samples(tag + "x", (B, Cc, HW, 1)))
    r = rnd(synth_input(tag + "r", (B, Cc, HW, 1))) if res else None
    cb = synth_input(tag + "cb", (B, Cc)) if cbias else None
    g = 1 + 0.2 * synth_input("gp_ga_g%d" % Cc, (Cc,))
    be = 0.3 * synth_input("gp_ga_b%d" % Cc, (Cc,))
    fn = {"none": lambda v: v, "silu": F.silu, "relu": F.relu}[act]

    def ref(ab, samples=None):
        sl = slice(None) if samples is None else samples
        y = fn(gn(x[sl], ab[sl], g, be))
        if cb is not None:
            y = y + cb[sl].double()[:, :, None, None]
        if r is not None:
            y = y + r[sl].double()
        return y

    return types.SimpleNamespace(id=tag + ("_res" if res else "") + ("_cb" if cbias else "") + "_" + act, kind="gn_apply", dt=dt,
                                 tol=1e-2 if dt == "bf16" else 1e-5, parts=PARTS, stored=x, count=Cc * HW, ref=ref, x=x, r=r, cb=cb,
                                 g=g, be=be, act=act, B=B, C=Cc, HW=HW)


@functools.lru_cache(maxsize=None)
def conv_case(mode, shape, cout, k=3, act="gelu", res=True, rc=None, halo=False):
    """act(conv_kxk(GN(x))) + res through ds_conv_igemm.  mode: "f32" / "bf16" (generic tiles and the bf16 halo kernel: x stored in
    that type, residual too), "x3" (split-precision halo kernel: x stored as hi + lo planes, fp32 residual).  rc = (c0, c1): the
    halo kernel's fused 1x1 res_conv over pad_and_concat(x0, x1) instead of a residual tensor (bf16)."""
    B, Cin, Hh, Ww = shape
    tag = "gp_cv_%s_%s_%d_%d" % (mode, "x".join(map(str, shape)), cout, k)
    rnd = {"f32": lambda t: t, "bf16": bf16r, "x3": split_sum}[mode]
    x = rnd(distinct_samples(tag + "x", shape))
    w = synth_input("gp_cv_w%d_%d_%d" % (cout, Cin, k), (cout, Cin, k, k), 0.05 if k == 3 else 0.1)
    b = synth_input("gp_cv_b%d" % cout, (cout,))
    g = 1 + 0.2 * synth_input("gp_cv_g%d" % Cin, (Cin,))
    be = 0.3 * synth_input("gp_cv_be%d" % Cin, (Cin,))
    r = None
    if res:
        r = synth_input(tag + "r", (B, cout, Hh, Ww))
        r = r if mode == "x3" else rnd(r)
    extra = None
    ns = types.SimpleNamespace()
    if rc is not None:
        c0, c1 = rc
        ns.wr = synth_input("gp_cv_wr%d" % (c0 + c1), (cout, c0 + c1, 1, 1), 0.1)
        ns.br = synth_input("gp_cv_br", (cout,))
        ns.x0 = bf16r(synth_input(tag + "x0", (B, c0, Hh, Ww)))
        ns.h1, ns.w1, ns.oh, ns.ow = Hh - 2, Ww - 1, 1, 0                     # decoder map short of the image: pad_and_concat offsets (1, 0)
        ns.x1 = bf16r(synth_input(tag + "x1", (B, c1, ns.h1, ns.w1))) if c1 else None
        xcat = ns.x0
        if c1:
            xcat = torch.cat([ns.x0, F.pad(ns.x1, (ns.ow, Ww - ns.w1 - ns.ow, ns.oh, Hh - ns.h1 - ns.oh))], 1)
        extra = F.conv2d(xcat.double(), ns.wr.double(), ns.br.double())
    fn = {"none": lambda v: v, "gelu": F.gelu}[act]
    pad = k // 2

    def tail(y):
        y = fn(y)
        if r is not None:
            y = y + r.double()
        if extra is not None:
            y = y + extra
        return y

    def ref(ab):
        return tail(F.conv2d(gn(x, ab, g, be), w.double(), b.double(), padding=pad))

    lin = []

    def ref_linear(ab):
        """The same operation through its linearity in (rstd, rstd * mean): three convolutions once, then any statistics for free."""
        if not lin:
            one = torch.ones(1, Cin, Hh, Ww, dtype=torch.float64)
            gd, bd = g.double().view(1, -1, 1, 1), be.double().view(1, -1, 1, 1)
            lin.append(F.conv2d(x.double() * gd, w.double(), padding=pad))
            lin.append(F.conv2d(one * gd, w.double(), padding=pad))
            lin.append(F.conv2d(one * bd, w.double(), b.double(), padding=pad))
        a, am = ab[:, 0].view(B, 1, 1, 1), ab[:, 1].view(B, 1, 1, 1)
        return tail(a * lin[0] - am * lin[1] + lin[2])

    ns.__dict__.update(id=tag + "_" + act + ("_res" if res else "") + ("_rc" if rc else ""), kind="conv", mode=mode,
                       tol={"f32": 2e-5, "bf16": 2e-2, "x3": 3e-5}[mode], parts=PARTS_HALO if halo else PARTS, stored=x, count=Cin * Hh * Ww,
                       ref=ref, ref_linear=ref_linear, x=x, w=w, b=b, g=g, be=be, r=r, act=act, shape=shape, cout=cout, k=k, rc=rc)
    return ns


def attn_spec(tag, Cc):
    return [(tag + ".fn.fn.to_qkv.weight", (384, Cc, 1, 1)), (tag + ".fn.fn.to_out.0.weight", (Cc, 128, 1, 1)),
            (tag + ".fn.fn.to_out.0.bias", (Cc,)), (tag + ".fn.fn.to_out.1.weight", (Cc,)), (tag + ".fn.fn.to_out.1.bias", (Cc,)),
            (tag + ".fn.fn.label_key.weight", (128, 512)), (tag + ".fn.fn.label_key.bias", (128,)),
            (tag + ".fn.fn.label_query.weight", (128, 512)), (tag + ".fn.fn.label_query.bias", (128,)),
            (tag + ".fn.norm.weight", (Cc,)), (tag + ".fn.norm.bias", (Cc,))]


@functools.lru_cache(maxsize=None)
def attn_case(mode, Cc, hw, cond, B=3):
    """Residual(PreNorm(LinearCrossAttentionAdd)) (oracle/unet_ref.py:attn_block) with the PreNorm's statistics GIVEN; the output
    GroupNorm takes the true statistics of its own input, as the kernels' finalize + ds_gn_apply route does.  mode "bf16" (x stored
    in bf16, ds_attn_fused_*) or "x3" (fp32 x, ds_attn_x3_*)."""
    from oracle import unet_ref as U
    Hh, Ww = hw
    tag = "gp_at%d" % Cc
    sd = synth_state_dict(attn_spec(tag, Cc))
    # (gain 0.5: the residual x then weighs against the attention branch about as in the existing attention tests, 1.7 : 1 — at gain 1
    # the large samples of x dominate both error norms and a fault in the branch moves them by 7 tolerances only)
    x = distinct_samples("gp_at_x%s_%d_%s" % (mode, Cc, hw), (B, Cc, Hh, Ww), 0.5)
    x = bf16r(x) if mode == "bf16" else x
    c = synth_input("gp_at_c", (B, 512)) if cond else None
    sdd = {k_: v.double() for k_, v in sd.items()}

    def ref(ab):
        y = gn(x, ab, sd[tag + ".fn.norm.weight"], sd[tag + ".fn.norm.bias"])
        return U.linear_attention(sdd, tag + ".fn.fn", y, c.double() if c is not None else None, "linear_add") + x.double()

    return types.SimpleNamespace(id="%s_%s_%d_%dx%d" % (tag, mode, Cc, Hh, Ww), kind="attn", mode=mode, tol=2e-2 if mode == "bf16" else 2e-5,
                                 parts=PARTS, stored=x, count=Cc * Hh * Ww, ref=ref, x=x, c=c, sd=sd, tag=tag, C=Cc, hw=hw, B=B)


FAST_C = (64, 96, 192, 384, 768)
FAST_HW = (5, 67, 600)                         # fewer pixels than `rows`, ragged against rows * 4, several blocks
GN_APPLY_FAST = [("bf16", c, hw, 3, res) for c in FAST_C for hw in FAST_HW for res in (False, True)]
GN_APPLY_CAP = ("bf16", 768, 520, 64, True)    # bx = 65 exceeds the grid cap 4096 / 64
GN_APPLY_LAZY = [("f32", 96, 70, 3, True, False, "none"), ("bf16", 160, 70, 3, False, True, "none"), ("bf16", 96, 70, 3, False, False, "silu")]

IGEMM = [(dt, (3, 96, 9, 7), 192, 3, "gelu", True) for dt in ("f32", "bf16")] + [(dt, (3, 96, 8, 16), 384, 1, "none", False) for dt in ("f32", "bf16")]
HALO_BF16 = [((3, 96, 8, 64), 192), ((3, 32, 33, 8), 96), ((3, 64, 7, 3), 96)]        # images 64, 8 and 3 wide
HALO_X3 = [((3, 96, 8, 64), 192), ((3, 96, 16, 8), 192), ((5, 32, 16, 5), 96), ((2, 64, 12, 7), 96)]
HALO_RC = ((2, 96, 9, 27), 96, (96, 96))
ATTN = [(96, (5, 10), False), (192, (33, 32), True), (384, (8, 6), True)]


def all_cases():
    """Every consumer launch of part A (the two halo output modes of a split-precision shape share their input: one entry each)."""
    for a in GN_APPLY_FAST:
        yield gn_apply_case(*a)
    yield gn_apply_case(*GN_APPLY_CAP)
    for a in GN_APPLY_LAZY:
        yield gn_apply_case(*a)
    for a in IGEMM:
        yield conv_case(*a)
    for shape, cout in HALO_BF16:
        yield conv_case("bf16", shape, cout, 3, "gelu", True, None, True)
    for shape, cout in HALO_X3:
        yield conv_case("x3", shape, cout, 3, "gelu", False, None, True)
        yield conv_case("x3", shape, cout, 3, "none", True, None, True)
    yield conv_case("bf16", HALO_RC[0], HALO_RC[1], 3, "none", False, HALO_RC[2], True)
    for mode in ("bf16", "x3"):
        for a in ATTN:
            yield attn_case(mode, *a)
