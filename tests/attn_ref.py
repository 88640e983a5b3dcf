"""Plain CPU side of the bit-exact fused-attention tests (tests/test_attn_ref_cpu.py without a GPU, tests/test_hip_attn_paths.py with one):
first the bf16 tier, ds_attn_fused_context / ds_attn_fused_output in both kernel generations (csrc/attn_fused.hip, csrc/attn_out2.hpp); the
split-precision tier (csrc/attn_x3.hip) follows in the second half of the file, with what differs there.

Why a case here is exact.  There is no qkv tensor to construct: keys, values and queries come out of the projection of x with the PreNorm
fold, so the case builder shapes x and to_qkv until the projection itself lands on values every softmax treats as 0 or 1.

  keys     Six 'key channels' of x hold 0 at a column's selected pixels and -(256 .. 384) elsewhere.  A k row reads one of them with w gamma = 2
           and the all-zero channel 12 with w gamma = -2: the raw accumulator is 0 at a selected pixel and <= -512 elsewhere, t1 = t2 = 0 for
           the row, so the fold shift is 0 = -a k_raw_max.  The kernels form the running maximum and the exponent's argument with the SAME fma
           (softmax_tile_step): fma(ga2, 0, 0) = 0, P = exp2(0) = 1 at a selected pixel; elsewhere the argument is a log2e k_raw <= -369 and
           v_exp_f32 returns 0 (it flushes below -126; the builder asks for -160).  A tile or segment WITHOUT a selected pixel has an
           unselected key as its own maximum: its partial is finite rubbish that the next tile's rescale by exp2(-369) = 0, resp. the
           combine's weight expf(-255) = 0, removes exactly.  Such tiles and segments are most of every case.
  queries  Six 'query channels' in the same way: a pixel selects ONE group of rows d (16, 8, 4, 2, 1 or 1 of them per head), whose pairs
           (raw accumulator, additive part) are both 0, hence bit-identical after fma(ga2, aq, sh); label_q = -400 removes half of every
           group of two or more, a different half per sample and head, so the label and its stride decide what is stored.  Counts and
           `scale` are powers of two: q~ = scale / count exactly.
  values   v rows are one- or two-hot over the data channels (small integers) with w gamma = +-1; t1, t2 of these rows are NOT zero, the
           v side carries the fold shift.  V (normalised: first generation; raw: second), P, the context operand, q~, Y and M_b hold at
           most 8 significant bits (asserted), so every bf16 pack inside the kernels is exact and BOTH generations meet one float64
           reference.  All rows d of a query group read the same key channel: their context rows are equal, Y = scale ctx[d] stays at 8 bits.
  sums     every accumulated sum is a sum of few-hot products of small integers: the margin against 2^24 units is reported per case.
  y        the final store is the one real rounding: 'wide' cases give y more than 8 bits, with exact ties (exact_ref.check_rounding);
           'small' cases keep y so small that the (sum, sum of squares) partials are exact integers in any grouping.

What exact data cannot hold: a rescale by a factor other than 0 or 1 (ga scales the softmax argument and v at once), the k and q fold shift
(zero here)."""
import math
from types import SimpleNamespace

import torch

import exact_ref as E

PARTF = 32 + 32 + 1024
LOG2E32 = float(torch.tensor(1.44269504088896340736, dtype=torch.float32))
KILL = 160.0              # log2-domain distance below the maximum at which the builder calls a weight zero (v_exp_f32 flushes below -126)
NKEY, NQRY, ZCH, DATA0 = 6, 6, 12, 13
Q_GROUPS = [(0, 16), (16, 24), (24, 28), (28, 30), (30, 31), (31, 32)]          # rows d' of a head per query group
KEY_COUNTS = [1, 2, 4, 1, 2, 4]                                                  # selected pixels per key channel (capped by N)


def cdiv(a, b):
    return (a + b - 1) // b


# ================================================================================================= launch arithmetic (attn_fused.hip, host part)
def group_t(C, N):
    return 2 if (C == 96 and N >= 4096) else 1


def out_blocks(ngroups, B, C):
    nb = (256 if C == 384 else 512) // B
    nb = max(1, min(nb, ngroups))
    per = cdiv(ngroups, nb)
    return cdiv(ngroups, per)


def attn_out2_blocks(N, B, C):
    ntiles = cdiv(N, 32)
    nw, per_cu = (4, 3) if C == 96 else (8, 1)
    nb = cdiv(256 * per_cu, B)
    nb = max(1, min(nb, cdiv(ntiles, nw)))
    per = cdiv(ntiles, nb)
    return cdiv(ntiles, per)


def fused_batch(B, hint):
    return hint if hint > 0 else B


def ctx2_exists(C, N):
    return C in (96, 192) or (C == 384 and N >= 1024)


def use_ctx2(B, N, C, gen, hint=0):
    if gen == 1 or not ctx2_exists(C, N):
        return False
    return gen == 2 or fused_batch(B, hint) >= 96


def use_out2(B, N, C, gen, hint=0, mfold=True):
    if gen == 1 or not mfold or C not in (96, 192):
        return False
    return gen == 2 or fused_batch(B, hint) >= (32 if C == 96 else 96)


def generations(B, N, C, gen, hint=0, mfold=True):
    return (1 if use_ctx2(B, N, C, gen, hint) else 0) | (2 if use_out2(B, N, C, gen, hint, mfold) else 0)


def segments_gen(B, N, C, gen):
    """ds_attn_fused_segments_gen (it looks at B alone: it has no batch_hint)."""
    ntiles = cdiv(N, 32)
    if use_ctx2(B, N, C, gen):
        s = (1024 if C == 384 else 2048) // max(B, 1)
        return max(1, min(s, 64, ntiles))
    return max(1, min(N // 128, 32))


def stats_parts(B, N, C, gen, hint=0, mfold=True):
    if use_out2(B, N, C, gen, hint, mfold):
        return attn_out2_blocks(N, fused_batch(B, hint), C)
    return out_blocks(cdiv(N, 32 * group_t(C, N)), fused_batch(B, hint), C)


CTX2_NW = {96: 4, 192: 8, 384: 8}          # waves = segments per block of attn_ctx2 (NSB == NW in all three instantiations)
OUT2_NW = {96: 4, 192: 8}


def ctx_form(B, N, C, gen, hint=0):
    """The context kernel a launch runs: ('ctx', NKS, T) or ('ctx2', NKS)."""
    if use_ctx2(B, N, C, gen, hint):
        return ("ctx2", C // 16)
    return ("ctx", C // 16, group_t(C, N))


def out_form(B, N, C, gen, hint=0, mfold=True):
    if use_out2(B, N, C, gen, hint, mfold):
        return ("out2", C // 16)
    return ("out", C // 16, group_t(C, N))


def ctx_segment_tiles(form, N, nseg):
    """Per segment, the 32-pixel tiles it walks, in order, as the kernel computes them.  First generation: whole groups of T tiles (a tile
    of the last group may lie wholly past N); second: tiles."""
    if form[0] == "ctx":
        T = form[2]
        ngroups = cdiv(N, 32 * T)
        per = cdiv(ngroups, nseg)
        out = []
        for s in range(nseg):
            g0, g1 = s * per, min(ngroups, s * per + per)
            out.append([g * T + t for g in range(g0, max(g0, g1)) for t in range(T)])
        return out
    ntiles = cdiv(N, 32)
    per = cdiv(ntiles, nseg)
    out = []
    for s in range(nseg):
        t0 = min(ntiles, s * per)
        out.append(list(range(t0, min(ntiles, t0 + per))))
    return out


def ctx_paths(form, N, nseg):
    """What a context launch exercises."""
    segs = ctx_segment_tiles(form, N, nseg)
    T = form[2] if form[0] == "ctx" else 1
    paths = set()
    groups = [len(s) // T for s in segs]
    if any(g == 0 for g in groups):
        paths.add("empty_segment")
    if any(g == 1 for g in groups):
        paths.add("one_group_segment")                     # the prefetch clamp g0 + 1 < g1
    if any(g > 1 and g % 2 == 1 for g in groups):
        paths.add("odd_groups")
    if any(g > 0 and g % 2 == 0 for g in groups):
        paths.add("even_groups")
    if N % 32:
        paths.add("ragged_last_tile")
    if sum(1 for g in groups if g) > 1:
        paths.add("several_segments")
    if sum(1 for g in groups if g) == 1 and nseg > 1:
        paths.add("all_but_one_empty")
    if form[0] == "ctx2" and nseg % CTX2_NW[form[1] * 16]:
        paths.add("wave_past_nseg")
    if T == 2 and 33 <= N % 64 <= 63:
        paths.add("t2_ragged_second_tile")
    if T == 2 and 1 <= N % 64 <= 31:
        paths.add("t2_second_tile_past_n")
    return paths


def out_block_tiles(form, N, C, batch):
    """Per block of the output pass, per wave (second generation) or as one list (first: the four waves walk the same groups), the tiles."""
    if form[0] == "out":
        T = form[2]
        ngroups = cdiv(N, 32 * T)
        nb = out_blocks(ngroups, batch, C)
        per = cdiv(ngroups, nb)
        return [[[g * T + t for g in range(i * per, min(ngroups, i * per + per)) for t in range(T)]] for i in range(nb)]
    nw = OUT2_NW[C]
    ntiles = cdiv(N, 32)
    nb = attn_out2_blocks(N, batch, C)
    per = cdiv(ntiles, nb)
    return [[list(range(i * per + w, min(ntiles, i * per + per), nw)) for w in range(nw)] for i in range(nb)]


def out_paths(form, N, C, batch):
    blocks = out_block_tiles(form, N, C, batch)
    T = form[2] if form[0] == "out" else 1
    paths = set()
    if N % 32:
        paths.add("ragged_last_tile")
    if len(blocks) > 1:
        paths.add("several_blocks")
    for blk in blocks:
        for w in blk:
            n = len(w) // T
            if n == 0:
                paths.add("wave_without_tile")
            if n > 1:
                paths.add("several_trips")
            if form[0] == "out":
                if n == 1:
                    paths.add("one_group_block")
                if n > 1 and n % 2:
                    paths.add("odd_groups")
                if n > 0 and n % 2 == 0:
                    paths.add("even_groups")
    if form[0] == "out" and len(blocks) == 1 and len(blocks[0][0]) // T > 2:
        paths.add("one_block_all_groups")                  # the prefetch clamp g + 2 < g1 over a long walk
    if T == 2 and 33 <= N % 64 <= 63:
        paths.add("t2_ragged_second_tile")
    if T == 2 and 1 <= N % 64 <= 31:
        paths.add("t2_second_tile_past_n")
    return paths


# ================================================================================================= the case builder
def _pow2_floor(n):
    return 1 << (n.bit_length() - 1)


def _is_pow2(t):
    t = t.to(torch.int64)
    return bool(((t > 0) & ((t & (t - 1)) == 0)).all())


def q_group_of(h, d):
    """(group index, query channel) of row d of head h: the groups are rotated by 8 rows per head, the channels by two."""
    dd = (d + 8 * h) % 32
    j = next(i for i, (lo, hi) in enumerate(Q_GROUPS) if lo <= dd < hi)
    return j, (j + 2 * h) % NQRY


def attn_case(C, B, N, wide=True, label=True, seed=0):
    """An exact case (module docstring).  Everything float64 on the CPU; `want_*` are what the device must store, bit for bit."""
    assert C in (96, 192, 384) and B >= 1 and N >= 1
    g = E.gen(1000 * C + 10 * N + B + 7919 * seed + (1 if wide else 0))
    c = SimpleNamespace(C=C, B=B, N=N, wide=wide, scale=0.25 if wide else 1.0, lq_stride=136,
                        id="C%d_B%d_N%d_%s%s" % (C, B, N, "wide" if wide else "small", "" if label else "_nolabel"))
    a, mean, gamma, beta = E.gn_numbers(g, B, C)
    c.a, c.mean = a.view(B), mean.view(B)
    beta[:DATA0] = 0.0
    if not wide:
        beta[:] = 0.0
    c.gamma, c.beta = gamma, beta
    # ---- x
    nd = C - DATA0
    xa = 3 if wide else 1
    x = torch.zeros(B, N, C, dtype=torch.float64)
    x[:, :, DATA0:] = E.ints(g, (B, N, nd), -xa, xa, density=1.0 if wide else 0.25)
    c.key_sel = torch.zeros(B, N, NKEY, dtype=torch.bool)
    for b in range(B):
        for j in range(NKEY):
            cnt = min(KEY_COUNTS[j] if wide else 1, _pow2_floor(N))
            pick = torch.randperm(N, generator=g)[:cnt].tolist()
            if j == 0:
                pick[0] = 0                                  # pixel 0: what the second generation's ragged lanes read
            if j == 1 and (cnt > 1 or N == 1):
                pick[0], pick[-1] = 0, N - 1                 # pixel 0 beside the last pixel: a ragged lane that reads pixel 0 again changes the mean
            if len(set(pick)) < cnt:                         # (the forced pixel was drawn already)
                pick = list(set(pick)) + [p for p in range(N) if p not in pick][:cnt - len(set(pick))]
            c.key_sel[b, pick, j] = True
    x[:, :, :NKEY] = torch.where(c.key_sel, 0.0, -(256.0 + 2.0 * torch.randint(0, 65, (B, N, NKEY), generator=g).double()))
    c.q_pick = torch.randint(0, NQRY, (B, N), generator=g)
    qsel = torch.nn.functional.one_hot(c.q_pick, NQRY).bool()
    x[:, :, NKEY:NKEY + NQRY] = torch.where(qsel, 0.0, -(512.0 + 4.0 * torch.randint(0, 65, (B, N, NQRY), generator=g).double()))
    c.x = x
    # ---- to_qkv: rows q | k | v
    w = torch.zeros(384, C, dtype=torch.float64)
    for h in range(4):
        for d in range(32):
            j, qc = q_group_of(h, d)
            kc = (j + h) % NKEY                              # all rows of a query group share one key channel: equal context rows
            for row, ch in ((h * 32 + d, NKEY + qc), (128 + h * 32 + d, kc)):
                w[row, ch] = 2.0 / gamma[ch]
                w[row, ZCH] = -2.0 / gamma[ZCH]
            e = d
            c1 = DATA0 + (7 * e + 3 * h) % nd
            c2 = DATA0 + (11 * e + 5 * h + 1) % nd
            w[256 + h * 32 + e, c1] = (1.0 if wide else 2.0) / gamma[c1]
            if wide and c2 != c1:
                w[256 + h * 32 + e, c2] = (-1.0 if (e + h) % 3 else 1.0) / gamma[c2]
    c.wqkv = w
    # ---- to_out: one entry per head and row (M_b = w ctx stays at 8 bits), bias
    wo = torch.zeros(C, 128, dtype=torch.float64)
    vals = [1.0, -1.0, 2.0, -2.0, 0.5, -0.5] if wide else [1.0, -1.0]
    for ch in range(C):
        for h in range(4):
            if wide or (ch + h) % 4 == 0:
                wo[ch, h * 32 + (ch * 7 + h * 5) % 32] = vals[(ch + h) % len(vals)]
    c.wout = wo
    c.bias = E.ints(g, (C,), -2, 2) if wide else E.ints(g, (C,), -1, 1, density=0.5)
    # ---- label_q: -400 on one half of every group of two or more rows
    c.label_full = None
    if label:
        lab = torch.full((B, c.lq_stride), float("nan"), dtype=torch.float64)
        lab[:, :128] = 0.0
        for b in range(B):
            for h in range(4):
                for (lo, hi) in Q_GROUPS:
                    if hi - lo >= 2:
                        half = (hi - lo) // 2
                        k0 = lo + (half if (b + h) % 2 else 0)
                        for dd in range(k0, k0 + half):
                            lab[b, h * 32 + (dd - 8 * h) % 32] = -400.0
        c.label_full = lab
    _expect(c)
    return c


def fold_tables(c):
    """t1 = W beta, t2 = W gamma over the UNPACKED weights (ds_conv_fold_tables with bias NULL), float64."""
    return c.wqkv @ c.beta, c.wqkv @ c.gamma


def _label(c, model=None):
    if c.label_full is None:
        return torch.zeros(c.B, 128, dtype=torch.float64)
    if model == "lq_stride_ignored":                       # sample b reads [b * 128, b * 128 + 128) of the strided array
        return c.label_full.flatten()[:c.B * 128].view(c.B, 128)
    return c.label_full[:, :128]


def _expect(c):
    """Preconditions (asserted) and the float64 expectation."""
    B, N, C = c.B, c.N, c.C
    c.wpk = c.wqkv * c.gamma.view(1, C)
    assert E.is_bf16(c.wpk) and E.is_bf16(c.x) and E.is_bf16(c.wout), "operands must be exact in bf16"
    c.t1, c.t2 = fold_tables(c)
    a, am = c.a.view(B, 1, 1), (c.a * c.mean).view(B, 1, 1)
    raw = torch.einsum("bnc,rc->bnr", c.x, c.wpk)                                     # [B][N][384]
    shift = c.t1.view(1, 1, 384) - am * c.t2.view(1, 1, 384)
    c.raw, c.shift = raw, shift
    c.margin_proj = ((c.x.abs() @ c.wpk.abs().T).amax() * c.a.max() + shift.abs().amax()).item() / 0.25
    # ---- keys: 0 at the maximum, fold shift 0, everything else dead
    kraw, ksh = raw[..., 128:256], shift[..., 128:256]
    assert float(ksh.abs().max()) == 0.0 and float(kraw.amax(1).abs().max()) == 0.0, "every key column's maximum is raw 0 with shift 0"
    c.ksel = kraw == 0.0                                                              # [B][N][128]
    dead = (a * LOG2E32) * kraw
    assert c.ksel.all() or float(dead[~c.ksel].max()) <= -KILL
    kcnt = c.ksel.sum(1)
    assert _is_pow2(kcnt), "selected pixels per column: a power of two"
    # ---- values
    c.vraw = raw[..., 256:]
    c.vnorm = a * c.vraw + shift[..., 256:]
    assert E.is_bf16(c.vraw) and E.is_bf16(c.vnorm), "V must be exact in bf16, raw and normalised"
    ks = c.ksel.double().view(B, N, 4, 32)
    ctx = torch.einsum("bnhd,bnhe->bhde", ks, c.vnorm.view(B, N, 4, 32))
    c.margin_ctx = (torch.einsum("bnhd,bnhe->bhde", ks, c.vnorm.abs().view(B, N, 4, 32)).amax().item()) / E.unit_of(c.vnorm)
    ctx = ctx / kcnt.view(B, 4, 32, 1)
    assert E.is_bf16(ctx), "the context operand must be exact in bf16"
    c.ctx64 = ctx
    c.want_ctx = ctx.float()
    # ---- the rest from the context
    _expect_out(c)
    E.check_exact(max(c.margin_proj, c.margin_ctx, c.margin_z))
    if c.wide:
        E.check_rounding(c.z64)


def _expect_out(c, model=None):
    """Output side of the expectation; `model`: a defect of the output pass (see DEFECTS) -> returns the changed y instead of filling c."""
    B, N, C = c.B, c.N, c.C
    a = c.a.view(B, 1, 1)
    lab = _label(c, model)
    qarg = a * c.raw[..., :128] + c.shift[..., :128] + lab.view(B, 1, 128)            # natural-log domain
    qh = qarg.view(B, N, 4, 32)
    top = qh.amax(3, keepdim=True)
    qsel = qh == top
    if model is None:
        assert float(top.abs().max()) == 0.0, "the selected rows hold raw 0 + additive 0: bit-identical after the fma"
        assert qsel.all() or float(((qh - top) * LOG2E32)[~qsel].max()) <= -KILL
        assert _is_pow2(qsel.sum(3))
        assert math.log2(c.scale) == round(math.log2(c.scale))
    scale = 1.0 if model == "scale_dropped" else c.scale
    qt = qsel.double() * (scale / qsel.sum(3, keepdim=True))
    wo = c.wout.view(C, 4, 32)
    if model == "wout_heads_swapped":
        wo = wo[:, [0, 2, 1, 3]]
    Y = torch.einsum("bhde,bnhd->bnhe", c.ctx64, qt)
    z = torch.einsum("che,bnhe->bnc", wo, Y) + (0.0 if model == "bias_dropped" else c.bias.view(1, 1, C))
    if model is not None:
        return z
    assert E.is_bf16(qt) and E.is_bf16(Y), "q~ and Y must be exact in bf16"
    mb = torch.einsum("che,bhde->bchd", wo, c.ctx64)
    assert E.is_bf16(mb), "M_b must be exact in bf16"
    c.mb64 = mb
    u = E.unit_of(z)
    c.margin_z = ((torch.einsum("che,bnhe->bnc", wo.abs(), Y.abs()) + c.bias.abs().view(1, 1, C)).amax().item()) / u
    c.z64 = z
    c.want_y = E.rne_bf16(z)
    # statistics: the first generation sums the fp32 values before the store, the second the stored bf16 values
    yd = c.want_y.double()
    c.stats_z = torch.stack([z.flatten(1).sum(1), (z * z).flatten(1).sum(1)], 1)
    c.stats_y = torch.stack([yd.flatten(1).sum(1), (yd * yd).flatten(1).sum(1)], 1)
    # exact in any grouping when sum |v| and sum v^2 stay below 2^24 units (units u and u^2) per sample
    c.stats_margin = max((z.abs().flatten(1).sum(1).max().item()) / u, ((z * z).flatten(1).sum(1).max().item()) / (u * u))
    c.stats_exact = c.stats_margin < E.LIMIT
    c.round_share, c.round_ties = E.rounding_profile(z)


def block_stats(c, form, batch, rounded):
    """[B][blocks][2] float64: the (sum, sum of squares) slot of every block of the output pass."""
    v = (c.want_y.double() if rounded else c.z64)
    blocks = out_block_tiles(form, c.N, c.C, batch)
    out = torch.zeros(c.B, len(blocks), 2, dtype=torch.float64)
    for i, blk in enumerate(blocks):
        for wv in blk:
            for t in wv:
                s = v[:, t * 32:min(c.N, t * 32 + 32)]
                out[:, i, 0] += s.flatten(1).sum(1)
                out[:, i, 1] += (s * s).flatten(1).sum(1)
    return out


def gn_partials(c, parts=3):
    """Raw (sum, sum of squares) partials [B][parts][2] fp32 and the (count, eps) with which the kernels' own reduction returns exactly
    (a, a mean): eps = 0, mean = s1 / count, var = s2 / count - mean^2 = 1 / a^2."""
    count = float(c.N * c.C)
    s1 = c.mean * count
    s2 = (1.0 / (c.a * c.a) + c.mean * c.mean) * count
    out = torch.zeros(c.B, parts, 2, dtype=torch.float64)
    for b in range(c.B):
        for j, tot in enumerate((s1[b].item(), s2[b].item())):
            first = math.floor(tot / parts)
            out[b, :, j] = first
            out[b, parts - 1, j] = tot - first * (parts - 1)
    assert E.is_f32(out) and torch.equal(out.sum(1)[:, 0], s1) and torch.equal(out.sum(1)[:, 1], s2)
    return out.float(), count, 0.0


# ================================================================================================= the context pass, step by step (fp32)
def _f32(t):
    return t.float().double()


def _exp2_hw(t):
    """v_exp_f32: 2^t in fp32, results below the normal range flushed to zero."""
    r = torch.exp2(t.float())
    return torch.where(t.float() < -126.0, torch.zeros_like(r), r).double()


def _half_of_row(r):
    return (r >> 2) & 1                                     # acc_row32: rows 0-3, 8-11, .. belong to lane half 0


def ctx_walk(c, form, nseg, defect=None):
    """The context pass as the kernels walk it: segments, tiles, the online softmax with every fp32 rounding point (values carried as
    float64 holding fp32 numbers), the partials, the combine.  Returns ctx [B][4][32][32] fp32.  `defect`: one step done wrong."""
    B, N, C = c.B, c.N, c.C
    gen2 = form[0] == "ctx2"
    T = 1 if gen2 else form[2]
    ga = c.a.view(B, 1)
    ga2 = _f32(ga * LOG2E32)
    shk = (c.shift[:, 0, 128:256])                           # [B][128]
    shk2 = _f32(shk * LOG2E32)
    shv = c.shift[:, 0, 256:].view(B, 4, 1, 32)
    kraw, vraw = c.raw[..., 128:256], c.raw[..., 256:]
    segs = ctx_segment_tiles(form, N, nseg)
    rows = torch.arange(32)
    half = _half_of_row(rows)                                # [32] lane half of a pixel row
    ehalf = _half_of_row(torch.arange(32))                   # ... and of a context row e
    pm, pl, pc = [], [], []
    for si, tiles in enumerate(segs):
        if defect == "drop_last_tile" and tiles:
            tiles = tiles[:-1]
        m = torch.full((B, 128, 2), float("-inf"), dtype=torch.float64)
        ls = torch.zeros(B, 128, 2, dtype=torch.float64)
        ctx = torch.zeros(B, 128, 32, dtype=torch.float64)  # [b][(h, d)][e]
        for t in tiles:
            px = t * 32 + rows
            real = px < N
            src = torch.where(real, px, torch.zeros_like(px))
            ak, av = kraw[:, src].clone(), vraw[:, src].clone()                       # [B][32][128]
            if not gen2:                                     # the first generation's stage holds zeros past N
                ak[:, ~real] = 0.0
                av[:, ~real] = 0.0
            masked = ~real
            if defect == "ragged_unmasked":
                masked = torch.zeros_like(real)
            if defect == "t2_first_tile_bound" and T == 2 and t % 2 == 1:
                masked = (px - 32) >= N                      # the second tile of a group masked with the first tile's bound
            ak[:, masked] = float("-inf")
            mr = torch.stack([ak[:, half == f].amax(1) if bool((half == f).any()) else ak.amax(1) for f in (0, 1)], -1)   # [B][128][2]
            if defect != "halves_max_not_shared":
                mr = mr.amax(-1, keepdim=True).expand(-1, -1, 2)
            mt = _f32(ga2.view(B, 1, 1) * mr + shk2.view(B, 128, 1))
            mn = torch.maximum(m, mt)
            assert defect is not None or bool(torch.isfinite(mn).all()), "a tile without a real pixel ahead of every real one"
            sc = _exp2_hw(_f32(m - mn))
            m = mn
            cexp = _f32(shk2.view(B, 128, 1) - mn)                                    # [B][128][2]
            arg = _f32(ga2.view(B, 1, 1) * ak + cexp[:, :, half].permute(0, 2, 1))    # [B][32 px][128]
            P = _exp2_hw(arg)
            V = av if gen2 else _f32(ga.view(B, 1, 1) * av + shv.expand(B, 4, 1, 32).reshape(B, 1, 128))
            Pb, Vb = P.float().bfloat16().double(), V.float().bfloat16().double()
            for f in (0, 1):
                ls[:, :, f] = _f32(ls[:, :, f] * sc[:, :, f] + P[:, half == f].sum(1))
            if defect != "rescale_skipped":
                ctx = ctx * sc[:, :, ehalf]                  # the factor is per lane: (d, half of e)
            ctx = _f32(ctx + torch.einsum("bphd,bphe->bhde", Pb.view(B, 32, 4, 32), Vb.view(B, 32, 4, 32)).reshape(B, 128, 32))
        lsum = ls.sum(-1)
        if gen2:                                             # v's normalisation applied once to the finished segment
            ctx = _f32(ga.view(B, 1, 1) * ctx + _f32(shv.expand(B, 4, 32, 32).reshape(B, 128, 32) * lsum.view(B, 128, 1)))
        if not tiles and defect == "stale_empty_segment" and pm:
            pm.append(pm[-1]); pl.append(pl[-1]); pc.append(pc[-1])
            continue
        pm.append(_f32(m[:, :, 0] * _f32(torch.tensor(1.0 / LOG2E32, dtype=torch.float64))))
        pl.append(lsum)
        pc.append(ctx)
    return combine(torch.stack(pm, 1), torch.stack(pl, 1), torch.stack(pc, 1)).view(B, 4, 32, 32)


def combine(pm, pl, pc):
    """attn_ctx_combine (linattn.hip) without a label token: pm, pl [B][nseg][128], pc [B][nseg][128][32] -> ctx [B][128][32] fp32."""
    M = pm.amax(1, keepdim=True)
    f = torch.exp((pm - M).float()).double()
    f = torch.where(torch.isnan(f), torch.zeros_like(f), f)
    Lr = torch.zeros_like(pl[:, 0])
    A = torch.zeros_like(pc[:, 0])
    for s in range(pm.shape[1]):
        Lr = _f32(Lr + _f32(f[:, s] * pl[:, s]))
        A = _f32(A + _f32(f[:, s].unsqueeze(-1) * pc[:, s]))
    return (A / Lr.unsqueeze(-1)).float()


def out_walk(c, form, ctx=None):
    """The output pass with every fp32 / bf16 rounding point of its kernel form (tiles are independent: all pixels at once).  First
    generation: q~ -> bf16, Y = ctx^T q~ -> bf16, Z = Wout Y + bias; second: M_b = Wout ctx^T -> bf16, Z = bias + M_b q~.  Returns y bf16."""
    B, N, C = c.B, c.N, c.C
    ctx = c.want_ctx.double() if ctx is None else ctx.double()
    bf = lambda t: t.float().bfloat16().double()
    ga2 = _f32(c.a.view(B, 1, 1) * LOG2E32)
    gam = (c.a * c.mean).view(B, 1)
    add = _f32(_f32(c.t1[:128].view(1, 128) - _f32(gam * c.t2[:128].view(1, 128))) + _label(c))
    shq = _f32(add * LOG2E32)
    q = _f32(ga2 * c.raw[..., :128] + shq.view(B, 1, 128)).view(B, N, 4, 32)
    e = _exp2_hw(_f32(q - q.amax(3, keepdim=True)))
    sq = _f32(e.sum(3, keepdim=True))
    qt = bf(_f32(e * _f32(c.scale / sq)))
    wo = c.wout.view(C, 4, 32)
    if form[0] == "out":
        Y = bf(_f32(torch.einsum("bhde,bnhd->bnhe", bf(ctx), qt)))
        z = _f32(_f32(torch.einsum("che,bnhe->bnc", wo, Y)) + c.bias.view(1, 1, C))
    else:
        mb = bf(_f32(torch.einsum("che,bhde->bchd", wo, ctx)))
        z = _f32(c.bias.view(1, 1, C) + torch.einsum("bchd,bnhd->bnc", mb, qt))
    return z.float().bfloat16()


# ================================================================================================= defect models
CTX_DEFECTS = ("ragged_unmasked", "drop_last_tile", "stale_empty_segment", "rescale_skipped", "halves_max_not_shared", "t2_first_tile_bound")
OUT_DEFECTS = ("wout_heads_swapped", "lq_stride_ignored", "scale_dropped", "bias_dropped")
GN_DEFECTS = ("gn_part_wrong_count",)
NOT_MODELLED = {
    "double-buffer parity swapped": "the wrong buffer of the first tile is LDS nobody wrote: a model would have to invent its content",
    "single-group prefetch reads group g0 + 1": "the group is loaded and never consumed: no stored value depends on it (an extent question, tools/bounds_sweep.py)",
    "wave with no tile stores": "it would store to addresses of another wave's tile or past N: seen by the device tests as a changed y or a broken guard word, not a value a model can name",
    "statistics slot of an idle block stale": "no launch of this tier has an idle block: blocks = ceil(n / ceil(n / nb)) leaves none without a tile (asserted for every case)",
}


def defect_y(c, model):
    """y (bf16) under an output-pass defect."""
    z = _expect_out(c, model)
    return z.float().bfloat16()                             # (a NaN label stays NaN: it compares unequal)


def gn_wrong_count(c):
    """The context (fp32) if gn_part were reduced with a count one element short: (a, a mean) move in their fifth digit."""
    part, count, eps = gn_partials(c)
    s = part.double().sum(1)
    cnt = count - 1.0
    mean = s[:, 0] / cnt
    var = (s[:, 1] / cnt - mean * mean).clamp_min(0.0)
    a = 1.0 / torch.sqrt(var + eps)
    a, am = a.float().double().view(-1, 1, 1), (a * mean).float().double().view(-1, 1, 1)
    vn = a * c.vraw + (c.t1[256:].view(1, 1, 128) - am * c.t2[256:].view(1, 1, 128))
    ks = c.ksel.double().view(c.B, c.N, 4, 32)
    return (torch.einsum("bnhd,bnhe->bhde", ks, vn.view(c.B, c.N, 4, 32)) / c.ksel.sum(1).view(c.B, 4, 32, 1)).float()


# ================================================================================================= the GPU cases
def _k(C, B, N, gen, nseg, hint=0, wide=True, label=True, mfold=True, gn="ab"):
    return dict(C=C, B=B, N=N, gen=gen, nseg=nseg, hint=hint, wide=wide, label=label, mfold=mfold, gn=gn)


def gpu_cases():
    """nseg: an int, or 'lib' (ds_attn_fused_segments_gen at B, resp. at the hint for gen = 0)."""
    cs = []
    # ---- attn_fused_ctx<6,1> / attn_fused_out<6,1>
    for N, B, nseg in ((1, 1, 1), (31, 2, 2), (32, 3, 1), (33, 1, 2), (64, 2, 3), (65, 3, 2), (127, 1, 8), (129, 2, 3), (257, 3, "lib"),
                       (257, 1, 3), (257, 2, 65)):
        cs.append(_k(96, B, N, 1, nseg, wide=(N % 2 == 1 and N > 1 and (B, N) != (3, 65))))
    cs.append(_k(96, 2, 257, 1, 2, hint=512))                                   # one block per sample walks all nine groups
    cs.append(_k(96, 1, 129, 1, 2, mfold=False, gn="part"))
    cs.append(_k(96, 2, 65, 1, 1, label=False, wide=False, gn="part"))
    # ---- <6,2>: 64-pixel groups from 4096 pixels on
    cs.append(_k(96, 1, 4129, 1, "lib", wide=False))                            # 4129 % 64 = 33: the second tile of the last group is ragged
    cs.append(_k(96, 1, 4101, 1, 3, wide=False))                                # 4101 % 64 = 5: the second tile lies past N
    cs.append(_k(96, 1, 4129, 1, 65, hint=512, wide=False))
    # ---- <12,1>, <24,1>
    for N, B, nseg in ((33, 2, 2), (129, 1, 3), (257, 3, "lib"), (65, 1, 8)):
        cs.append(_k(192, B, N, 1, nseg, wide=(B != 3)))
        cs.append(_k(384, B, N, 1, nseg, wide=(B != 3)))
    cs.append(_k(192, 1, 257, 1, 2, hint=512, gn="part"))
    cs.append(_k(384, 1, 257, 1, 2, hint=256))
    cs.append(_k(192, 2, 257, 1, 3, hint=200))                                  # blocks of the output pass that walk an even number of groups
    # ---- second generation: attn_ctx2<6,4,4,1> + attn_out2<6,4>, <12,8,4,1> + <12,8>
    for C in (96, 192):
        for N, B, nseg in ((1, 1, 1), (33, 2, 2), (65, 3, 3), (129, 1, 8), (257, 2, "lib"), (257, 1, 65), (1056, 1, 3)):
            cs.append(_k(C, B, N, 2, nseg, wide=(N in (33, 129) or (B, N) == (1, 257) or (C, N) == (192, 65))))
    cs.append(_k(96, 2, 129, 2, 2, wide=False))                                 # segments of three and two tiles: an even walk
    cs.append(_k(192, 2, 129, 2, 2, wide=False))
    cs.append(_k(96, 2, 1056, 2, "lib", hint=512, wide=False, gn="part"))       # batch 512: one out2 block per sample, several trips per wave
    cs.append(_k(192, 1, 1056, 2, 8, hint=256, wide=False))
    # ---- <24,8,2,2>: C = 384 from 1024 pixels on (the output pass stays first generation)
    cs.append(_k(384, 1, 1056, 2, 3, wide=False))
    cs.append(_k(384, 2, 1056, 2, "lib", wide=False, gn="part"))
    cs.append(_k(384, 1, 1056, 2, 65, wide=False))
    cs.append(_k(384, 1, 1057, 2, 8, wide=False))                               # (1056 = 33 tiles exactly: one more pixel for a ragged last tile)
    # ---- gen = 0 on each side of each threshold
    for C, hint in ((96, 31), (96, 32), (96, 95), (96, 96), (192, 95), (192, 96)):
        cs.append(_k(C, 2, 129, 0, "lib", hint=hint))
    cs.append(_k(96, 2, 129, 0, "lib", hint=256, mfold=False))                  # mfold NULL keeps the first-generation output pass
    cs.append(_k(384, 1, 1056, 0, "lib", hint=96, wide=False))                  # C = 384: second-generation context, first-generation output
    cs.append(_k(384, 1, 1056, 0, "lib", hint=95, wide=False))                  # ... and just below the context threshold: both first generation
    cs.append(_k(384, 1, 257, 0, "lib", hint=96))                               # ... which does not exist below 1024 pixels
    return cs


def case_id(k):
    return "C%d_B%d_N%d_gen%d_s%s_h%d_%s%s%s_%s" % (k["C"], k["B"], k["N"], k["gen"], k["nseg"], k["hint"], "wide" if k["wide"] else "small",
                                                  "" if k["label"] else "_nolabel", "" if k["mfold"] else "_nomfold", k["gn"])


def resolve_nseg(k):
    if k["nseg"] != "lib":
        return k["nseg"]
    if k["gen"] == 0:                                       # the caller's rule (header): segments at the batch the decisions look at
        return segments_gen(fused_batch(k["B"], k["hint"]), k["N"], k["C"], 0)
    return segments_gen(k["B"], k["N"], k["C"], k["gen"])


_CASES = {}


def build(k):
    key = (k["C"], k["B"], k["N"], k["wide"], k["label"])
    if key not in _CASES:
        _CASES[key] = attn_case(k["C"], k["B"], k["N"], wide=k["wide"], label=k["label"])
    return _CASES[key]


def forms(k):
    batch = fused_batch(k["B"], k["hint"])
    return ctx_form(k["B"], k["N"], k["C"], k["gen"], k["hint"]), out_form(k["B"], k["N"], k["C"], k["gen"], k["hint"], k["mfold"]), batch


# =================================================================================================================================================
# The split-precision tier (csrc/attn_x3.hip): ds_attn_x3_context / ds_attn_x3_output on fp32 tensors, every dense product as
# x_hi w_hi + x_lo w_hi + x_hi w_lo.  The same construction of keys and queries; what differs is where the bits go.  The fp32 chain
# x -> V -> ctx -> M_b -> Z keeps every intermediate exact only while (largest magnitude) / (absolute unit) stays below 2^24 at EVERY link, and
# each operand with a lo part costs the next link eight or more bits.  No single case can afford a lo part everywhere, so three flavours:
#   'wlo'    the v rows of W gamma are +-(1 + 2^-8) (hi = 1, lo = 2^-8), x data are 9-10-bit integers (lo != 0) on the narrow channels and
#            17-20-bit integers (a third part is dropped) on the wide ones, which only the rows e = 31 read with weight 1; V, ctx and M_b
#            carry lo parts; scale = 1/4 (q~ has no lo part).
#   'qlo'    scale = 1/4 + 2^-10 (q~ = scale / count has a lo part), x data odd 9-bit integers (lo = +-1), plain +-1 weights: M_b stays at 12 bits.
#   'small'  the bf16 tier's small flavour on fp32 tensors: no lo part anywhere, every (sum, sum of squares) partial an exact integer - the
#            statistics slots and form B (which normalises with them) are then known bit for bit.
# For 'wlo' and 'qlo' the statistics are bounded, and form B is checked against the float64 value formed from the partials the device stored.
X3_DATA0 = 13
X3_Q_GROUPS = [(0, 8), (8, 16), (16, 24), (24, 28), (28, 30), (30, 32)]
NW3 = 8
QLO_SCALE = 0.25 + 2.0 ** -10


def z_tiles_per_block(N, B, C):
    ntiles, groups = cdiv(N, 32), C // 96
    nb = cdiv(256, B * groups)
    nb = max(1, min(nb, cdiv(ntiles, NW3)))
    return cdiv(ntiles, nb)


def x3_segments(B, N, C):
    ntiles, groups = cdiv(N, 32), (4 if C == 384 else 2)
    s = (2048 // groups) // max(B, 1)
    s = min(max(s, NW3), 128, ntiles)
    return max(s, 1)


def x3_stats_parts(B, N, C, hint=0):
    per = z_tiles_per_block(N, fused_batch(B, hint), C)
    return cdiv(cdiv(N, 32), per) * (C // 96)


def x3_q_only_segments(B, N, C):
    """launch_pass1's own count for the q-only launch (C = 192: four heads per block, C = 384: two).  From B, never from batch_hint; it
    decides which wave projects which tile and no stored bit (the q planes are per tile)."""
    hb = 4 if C == 192 else 2
    nseg = cdiv(2048 // (4 // hb), B)
    nseg = cdiv(nseg, NW3) * NW3
    return min(nseg, cdiv(N, 32))


def x3_pass1_tiles(N, nseg):
    """Per segment = wave, the tiles of attn_x3_pass1 (consecutive)."""
    return ctx_segment_tiles(("ctx2", 0), N, nseg)


def x3_ctx_paths(C, N, nseg, B=1):
    segs = x3_pass1_tiles(N, nseg)
    paths = set()
    n = [len(s) for s in segs]
    if any(v == 0 for v in n):
        paths.add("empty_segment")
    if any(v == 1 for v in n):
        paths.add("one_group_segment")
    if any(v > 1 and v % 2 for v in n):
        paths.add("odd_groups")
    if any(v > 0 and v % 2 == 0 for v in n):
        paths.add("even_groups")
    if N % 32:
        paths.add("ragged_last_tile")
    if nseg % NW3:
        paths.add("wave_past_nseg")
    if sum(1 for v in n if v) > 1:
        paths.add("several_segments")
    if C != 96:
        nq = x3_q_only_segments(B, N, C)                   # (launch_pass1 takes it from p->B)
        if any(len(s) == 0 for s in x3_pass1_tiles(N, nq)) or nq % NW3:
            paths.add("q_only_wave_without_tile")
    return paths


def x3_out_block_tiles(N, C, batch):
    """Per block (tile range; the C / 96 channel groups of attn_x3_z walk the same tiles), per wave, the tiles of pass 2."""
    ntiles = cdiv(N, 32)
    per = z_tiles_per_block(N, batch, C)
    nb = cdiv(ntiles, per)
    return [[list(range(i * per + w, min(ntiles, i * per + per), NW3)) for w in range(NW3)] for i in range(nb)]


def x3_out_paths(N, C, batch):
    blocks = x3_out_block_tiles(N, C, batch)
    paths = set()
    if N % 32:
        paths.add("ragged_last_tile")
    if len(blocks) > 1:
        paths.add("several_blocks")
    for blk in blocks:
        for w in blk:
            if not w:
                paths.add("wave_without_tile")
            if len(w) > 1:
                paths.add("several_trips")
            if len(w) > 1 and len(w) % 2:
                paths.add("odd_trips")
    return paths


def prod3(x, w, drop=None):
    """x w^T in the documented algebra, float64; drop = 'x_lo' leaves out x_lo w_hi."""
    xh, xl = E.split_hi_lo(x)
    wh, wl = E.split_hi_lo(w)
    r = xh @ wh.T + xh @ wl.T
    return r if drop == "x_lo" else r + xl @ wh.T


def x3_q_group_of(h, d):
    dd = (d + 8 * h) % 32
    j = next(i for i, (lo, hi) in enumerate(X3_Q_GROUPS) if lo <= dd < hi)
    return j, (j + 2 * h) % NQRY


def x3_case(C, B, N, flavour="wlo", label=True, seed=0):
    assert flavour in ("wlo", "qlo", "small")
    if flavour == "small":
        c = attn_case(C, B, N, wide=False, label=label, seed=seed)
        c.flavour, c.id = "small", "x3_C%d_B%d_N%d_small%s" % (C, B, N, "" if label else "_nolabel")
        c.q_groups = Q_GROUPS
        _x3_expect(c)
        return c
    g = E.gen(5000 * C + 10 * N + B + 7919 * seed + (3 if flavour == "wlo" else 4))
    c = SimpleNamespace(C=C, B=B, N=N, flavour=flavour, wide=True, scale=0.25 if flavour == "wlo" else QLO_SCALE, lq_stride=136, q_groups=X3_Q_GROUPS,
                        id="x3_C%d_B%d_N%d_%s%s" % (C, B, N, flavour, "" if label else "_nolabel"))
    a, mean, gamma, beta = E.gn_numbers(g, B, C)
    c.a, c.mean = a.view(B), mean.view(B)
    beta[:X3_DATA0] = 0.0
    c.gamma, c.beta = gamma, beta
    nd = C - X3_DATA0
    nwide = 10 * (C // 96) if flavour == "wlo" else 0
    nn = nd - nwide                                          # narrow data channels
    x = torch.zeros(B, N, C, dtype=torch.float64)
    sign = lambda shape: torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    if flavour == "wlo":
        x[:, :, X3_DATA0:X3_DATA0 + nn] = sign((B, N, nn)) * E.ints(g, (B, N, nn), 256, 639)
        x[:, :, X3_DATA0 + nn:] = sign((B, N, nwide)) * E.ints(g, (B, N, nwide), 1 << 16, (1 << 20) - 1)
    else:
        x[:, :, X3_DATA0:] = sign((B, N, nd)) * E.ints(g, (B, N, nd), 513, 1023)
    c.key_sel = torch.zeros(B, N, NKEY, dtype=torch.bool)
    for b in range(B):
        for j in range(NKEY):
            cnt = min(1 + j % 2, _pow2_floor(N)) if flavour == "wlo" else 1
            pick = torch.randperm(N, generator=g)[:cnt].tolist()
            if j == 0:
                pick[0] = 0
            if j == 1 and (cnt > 1 or N == 1):
                pick[0], pick[-1] = 0, N - 1                 # pixel 0 beside the last pixel: a ragged lane that reads pixel 0 again changes the mean
            if len(set(pick)) < cnt:
                pick = list(set(pick)) + [p for p in range(N) if p not in pick][:cnt - len(set(pick))]
            c.key_sel[b, pick, j] = True
    x[:, :, :NKEY] = torch.where(c.key_sel, 0.0, -(513.0 + 2.0 * torch.randint(0, 65, (B, N, NKEY), generator=g).double()))
    c.q_pick = torch.randint(0, NQRY, (B, N), generator=g)
    qsel = torch.nn.functional.one_hot(c.q_pick, NQRY).bool()
    x[:, :, NKEY:NKEY + NQRY] = torch.where(qsel, 0.0, -(1025.0 + 4.0 * torch.randint(0, 65, (B, N, NQRY), generator=g).double()))
    c.x = x
    w = torch.zeros(384, C, dtype=torch.float64)
    wv = (1.0 + 2.0 ** -8) if flavour == "wlo" else 1.0
    for h in range(4):
        for d in range(32):
            j, qc = x3_q_group_of(h, d)
            kc = (j + h) % NKEY
            for row, ch in ((h * 32 + d, NKEY + qc), (128 + h * 32 + d, kc)):
                w[row, ch] = 2.0 / gamma[ch]
                w[row, ZCH] = -2.0 / gamma[ZCH]
            e = d
            if flavour == "wlo" and e == 31:
                ch = X3_DATA0 + nn + h % nwide
                w[256 + h * 32 + e, ch] = 1.0 / gamma[ch]
            else:
                ch = X3_DATA0 + (7 * e + 3 * h) % nn
                w[256 + h * 32 + e, ch] = (-wv if (e + h) % 3 == 0 else wv) / gamma[ch]
    c.wqkv = w
    wo = torch.zeros(C, 128, dtype=torch.float64)
    vals = [1.0, -1.0, -1.0, 1.0]
    for ch in range(C):
        for h in range(4):
            if flavour == "wlo" and ch % 8 == 7 and h != (ch // 8) % 4:
                continue                                     # a channel of the wide rows takes ONE head: Z stays below 2^24 units
            e = 31 if (flavour == "wlo" and ch % 8 == 7) else (ch * 7 + h * 5) % 31
            wo[ch, h * 32 + e] = vals[(ch + h) % 4]
    c.wout = wo
    c.bias = E.ints(g, (C,), -2, 2)
    c.label_full = None
    if label:
        lab = torch.full((B, c.lq_stride), float("nan"), dtype=torch.float64)
        lab[:, :128] = 0.0
        for b in range(B):
            for h in range(4):
                for (lo, hi) in X3_Q_GROUPS:
                    half = (hi - lo) // 2
                    k0 = lo + (half if (b + h) % 2 else 0)
                    for dd in range(k0, k0 + half):
                        lab[b, h * 32 + (dd - 8 * h) % 32] = -400.0
        c.label_full = lab
    _x3_expect(c)
    return c


def _x3_chain(c, model=None):
    """The float64 value of the documented algebra from x to Z; `model`: one lo term dropped.  Returns (ctx, M_b, Z) and fills nothing."""
    B, N, C = c.B, c.N, c.C
    wpk = c.wqkv * c.gamma.view(1, C)
    t1, t2 = c.wqkv @ c.beta, c.wqkv @ c.gamma
    a, am = c.a.view(B, 1, 1), (c.a * c.mean).view(B, 1, 1)
    raw = torch.stack([prod3(c.x[b], wpk, drop="x_lo" if model == "x_lo_w_hi_dropped" else None) for b in range(B)])
    shift = t1.view(1, 1, 384) - am * t2.view(1, 1, 384)
    kraw = raw[..., 128:256]
    ksel = kraw == kraw.amax(1, keepdim=True)
    vraw = raw[..., 256:]
    vh, vl = E.split_hi_lo(vraw)
    v2 = vh if model == "v_lo_dropped" else vh + vl           # P is 0 or 1: hi = P, lo = 0
    ks = ksel.double().view(B, N, 4, 32)
    cnt = ksel.sum(1).view(B, 4, 32, 1)
    ctx = (a.view(B, 1, 1, 1) * torch.einsum("bnhd,bnhe->bhde", ks, v2.view(B, N, 4, 32)) + shift[:, 0, 256:].view(B, 4, 1, 32) * cnt) / cnt
    lab = torch.nan_to_num(_label(c, model), nan=0.0)      # (the defect model reads the NaN of the gap: any finite stand-in shows the change)
    qarg = a * raw[..., :128] + shift[..., :128] + lab.view(B, 1, 128)
    qh_ = qarg.view(B, N, 4, 32)
    qsel = qh_ == qh_.amax(3, keepdim=True)
    qt = qsel.double() * (c.scale / qsel.sum(3, keepdim=True))
    mb = torch.einsum("che,bhde->bchd", c.wout.view(C, 4, 32), ctx)
    mh, ml = E.split_hi_lo(mb)
    qh, ql = E.split_hi_lo(qt)
    if model == "mb_lo_dropped":
        ml = torch.zeros_like(ml)
    if model == "q_lo_dropped":
        ql = torch.zeros_like(ql)
    z = c.bias.view(1, 1, C) + torch.einsum("bchd,bnhd->bnc", mh + ml, qh) + torch.einsum("bchd,bnhd->bnc", mh, ql)
    return SimpleNamespace(raw=raw, shift=shift, ksel=ksel, qsel=qsel, vraw=vraw, ctx=ctx, mb=mb, mh=mh, ml=ml, qt=qt, qh=qh, ql=ql, z=z, wpk=wpk, t1=t1, t2=t2)


def _x3_expect(c):
    B, N, C = c.B, c.N, c.C
    r = _x3_chain(c)
    assert E.is_f32(c.x) and E.is_f32(r.wpk) and E.is_f32(c.wout)
    c.wpk, c.t1, c.t2, c.raw, c.shift = r.wpk, r.t1, r.t2, r.raw, r.shift
    a = c.a.view(B, 1, 1)
    kraw = r.raw[..., 128:256]
    assert float(r.shift[..., 128:256].abs().max()) == 0.0 and float(kraw.amax(1).abs().max()) == 0.0
    assert r.ksel.all() or float(((a * LOG2E32) * kraw)[~r.ksel].max()) <= -KILL
    assert _is_pow2(r.ksel.sum(1)) and _is_pow2(r.qsel.sum(3))
    qh_ = (a * r.raw[..., :128] + r.shift[..., :128] + _label(c).view(B, 1, 128)).view(B, N, 4, 32)
    top = qh_.amax(3, keepdim=True)
    assert float(top.abs().max()) == 0.0 and (r.qsel.all() or float(((qh_ - top) * LOG2E32)[~r.qsel].max()) <= -KILL)
    c.ksel3, c.vraw3 = r.ksel, r.vraw
    # margins: per output column, the largest sum of the magnitudes of its terms over the finest unit among them (absolute units: a part of
    # an operand is a multiple of the unit of the operand it was split from, whatever its own size)
    xh, xl = E.split_hi_lo(c.x)
    wh, wl = E.split_hi_lo(r.wpk)
    ux = [(_unit0(xh[..., ch]), _unit0(xl[..., ch])) for ch in range(C)]
    amin, amax = c.a.min().item(), c.a.max().item()
    proj = (xh.abs() + xl.abs()) @ wh.abs().T + xh.abs() @ wl.abs().T
    c.margin_proj = 0.0
    for row in range(384):
        u = _unit0(r.shift[..., row])
        for ch in r.wpk[row].nonzero().flatten().tolist():
            uwh, uwl = _unit0(wh[row, ch]), _unit0(wl[row, ch])
            u = min(u, amin * min(ux[ch][0] * uwh, ux[ch][1] * uwh, ux[ch][0] * uwl))
        c.margin_proj = max(c.margin_proj, (amax * proj[..., row].amax().item() + r.shift[..., row].abs().amax().item()) / u)
    assert E.is_f32(r.raw) and E.is_f32(r.ctx) and E.is_f32(r.mb) and E.is_f32(r.z), "an intermediate of the chain is not exact in fp32"
    vh, vl = E.split_hi_lo(r.vraw)
    ks = r.ksel.double().view(B, N, 4, 32)
    sv = torch.einsum("bnhd,bnhe->bhde", ks, (vh.abs() + vl.abs()).view(B, N, 4, 32)) * c.a.view(B, 1, 1, 1) \
        + r.shift[:, 0, 256:].abs().view(B, 4, 1, 32) * r.ksel.sum(1).view(B, 4, 32, 1)
    c.margin_ctx = max(sv[:, h, :, e].amax().item() / min(amin * _unit0(vh.view(B, N, 4, 32)[:, :, h, e]), amin * _unit0(vl.view(B, N, 4, 32)[:, :, h, e]),
                                                          _unit0(r.shift[:, 0, 256 + h * 32 + e])) for h in range(4) for e in range(32))
    uq = (_unit0(r.qh), _unit0(r.ql))
    sz = torch.einsum("bchd,bnhd->bnc", r.mh.abs() + r.ml.abs(), r.qh.abs()) + torch.einsum("bchd,bnhd->bnc", r.mh.abs(), r.ql.abs()) + c.bias.abs().view(1, 1, C)
    c.margin_z = max(sz[..., ch].amax().item() / min(_unit0(c.bias[ch]), _unit0(r.mh[:, ch]) * uq[0], _unit0(r.ml[:, ch]) * uq[0], _unit0(r.mh[:, ch]) * uq[1])
                     for ch in range(C))
    assert max(c.margin_proj, c.margin_ctx, c.margin_z) < E.LIMIT, "margins proj %.3g ctx %.3g z %.3g of 2^24" % (c.margin_proj / E.LIMIT, c.margin_ctx / E.LIMIT, c.margin_z / E.LIMIT)
    c.ctx64, c.mb64, c.z64 = r.ctx, r.mb, r.z
    c.want_ctx, c.want_y = r.ctx.float(), r.z.float()
    c.want_mfold = torch.stack([E.rne_bf16(r.mh), E.rne_bf16(r.ml)], 1)          # [B][2][C][4][32]
    z = r.z
    c.stats_z = torch.stack([z.flatten(1).sum(1), (z * z).flatten(1).sum(1)], 1)
    u_z = _unit_pow2(z)
    c.stats_margin = max((z.abs().flatten(1).sum(1).max().item()) / u_z, ((z * z).flatten(1).sum(1).max().item()) / (u_z * u_z))
    c.stats_exact = c.stats_margin < E.LIMIT
    # the shares of precondition 5
    c.share = dict(x_lo=E.split_profile(c.x)[0], x_wide3=E.split_profile(c.x)[1], wv_lo=E.split_profile(r.wpk[256:][r.wpk[256:] != 0])[0],
                   v_lo=E.split_profile(r.vraw[r.ksel.view(B, N, 4, 32).any(3).repeat_interleave(32, 2)])[0], mb_lo=E.split_profile(r.mb)[0],
                   q_lo=E.split_profile(r.qt[r.qt != 0])[0])
    if c.flavour == "wlo":
        E.check_lo_share(c.x, 0.5, "x")
        E.check_wide3(c.x)
        assert c.share["wv_lo"] >= 0.9 and c.share["v_lo"] >= 0.5 and c.share["mb_lo"] >= 0.5, c.share
    if c.flavour == "qlo":
        E.check_lo_share(c.x, 0.5, "x")
        assert c.share["q_lo"] == 1.0 and c.share["v_lo"] >= 0.5 and c.share["mb_lo"] >= 0.5, c.share
    if c.flavour == "small":
        assert c.stats_exact


def _unit0(t):
    """_unit_pow2, with an all-zero tensor counting as coarse (it adds nothing)."""
    t = torch.as_tensor(t, dtype=torch.float64)
    return _unit_pow2(t) if float(t.abs().max()) else 2.0 ** 30


def _unit_pow2(q):
    """unit_of for values that may be far below 1 (q~ parts): the largest power of two of which every element is a multiple."""
    q = torch.as_tensor(q, dtype=torch.float64)
    u = 2.0 ** 24
    while not torch.equal(q / u, (q / u).round()):
        u /= 2
        assert u >= 2.0 ** -40
    return u


def x3_block_stats(c, batch, v=None):
    """[B][parts][2] float64: slot (tile block tb, channel group cg) = tb * (C / 96) + cg of pass 2 (MODE 0 and MODE 1 alike)."""
    v = c.z64 if v is None else v
    blocks = x3_out_block_tiles(c.N, c.C, batch)
    gz = c.C // 96
    out = torch.zeros(c.B, len(blocks) * gz, 2, dtype=torch.float64)
    for i, blk in enumerate(blocks):
        for wv in blk:
            for t in wv:
                for cg in range(gz):
                    s = v[:, t * 32:min(c.N, t * 32 + 32), cg * 96:cg * 96 + 96]
                    out[:, i * gz + cg, 0] += s.flatten(1).sum(1)
                    out[:, i * gz + cg, 1] += (s * s).flatten(1).sum(1)
    return out


def x3_form_b(c, slots, on_gamma, on_beta, eps, y=None, split=E.split_hi_lo):
    """out = x + GroupNorm(y) as MODE 2 forms it from the partials `slots` [B][parts][2] (fp32 values): the kernels' float64 finish
    (gn_rstd_pair), the scale row a gamma_c and the shift row beta_c - a mean gamma_c (gamma a power of two: both products exact), one fma,
    one add.  Returns (out fp32, hi plane, lo plane)."""
    B, N, C = c.B, c.N, c.C
    y = c.want_y.double() if y is None else y.double()
    s = slots.double().sum(1)
    count = float(C * N)
    mean = s[:, 0] / count
    var = (s[:, 1] / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    oa, oam = rstd.float().double().view(B, 1, 1), (rstd * mean).float().double().view(B, 1, 1)
    sc = _f32(oa * on_gamma.view(1, 1, C))
    sh = _f32(on_beta.view(1, 1, C) - oam * on_gamma.view(1, 1, C))
    p = y * sc                                               # exact: 24 x 24 bits
    t = p + sh                                               # one float64 rounding in front of the fp32 one: refuse the cases where it could matter
    bb = t - p
    err = (p - (t - bb)) + (sh - bb)                         # TwoSum: the part of p + sh that t lost
    low = t.contiguous().view(torch.int64) & ((1 << 29) - 1)
    assert not bool(((err != 0) & ((low - (1 << 28)).abs() <= 1)).any()), "an inexact float64 sum within an ulp of an fp32 tie: the fma cannot be restated"
    out = _f32(c.x + _f32(t))
    hi, lo = split(out)
    return out.float(), hi.float().bfloat16(), lo.float().bfloat16()


X3_DEFECTS = ("x_lo_w_hi_dropped", "v_lo_dropped", "mb_lo_dropped", "q_lo_dropped", "lq_stride_ignored", "form_b_stats_of_pass2", "out_planes_lo_truncated")


def x3_defect_y(c, model):
    return _x3_chain(c, model).z.float()


def x3_ctx_walk(c, nseg, defect=None):
    """attn_x3_pass1 (k / v launch) step by step: a wave = a segment of consecutive tiles, raw V, P and V split into hi / lo for ctx^T += V^T P
    in three terms, v's normalisation applied to the finished segment; then the combine.  Returns ctx fp32."""
    B, N = c.B, c.N
    ga = c.a.view(B, 1)
    ga2 = _f32(ga * LOG2E32)
    shk2 = _f32(c.shift[:, 0, 128:256] * LOG2E32)
    shv = c.shift[:, 0, 256:].view(B, 4, 1, 32).expand(B, 4, 32, 32).reshape(B, 128, 32)
    kraw, vraw = c.raw[..., 128:256], c.raw[..., 256:]
    rows = torch.arange(32)
    pm, pl, pc = [], [], []
    for tiles in x3_pass1_tiles(N, nseg):
        if defect == "drop_last_tile" and tiles:
            tiles = tiles[:-1]
        m = torch.full((B, 128), float("-inf"), dtype=torch.float64)
        ls = torch.zeros(B, 128, dtype=torch.float64)
        ctx = torch.zeros(B, 128, 32, dtype=torch.float64)
        for t in tiles:
            px = t * 32 + rows
            real = px < N
            src = torch.where(real, px, torch.zeros_like(px))
            ak, av = kraw[:, src].clone(), vraw[:, src].clone()
            if defect != "ragged_unmasked":
                ak[:, ~real] = float("-inf")
            mn = torch.maximum(m, _f32(ga2.view(B, 1) * ak.amax(1) + shk2))
            sc = _exp2_hw(_f32(m - mn))
            m = mn
            P = _exp2_hw(_f32(ga2.view(B, 1, 1) * ak + _f32(shk2 - mn).view(B, 1, 128)))
            ls = _f32(ls * sc + P.sum(1))
            if defect != "rescale_skipped":
                ctx = ctx * sc.unsqueeze(-1)
            ph, pl_ = (lambda h: (h, (P - h).float().bfloat16().double()))(P.float().bfloat16().double())
            vh = av.float().bfloat16().double()
            vl = (av - vh).float().bfloat16().double()
            e3 = lambda p_, v_: torch.einsum("bphd,bphe->bhde", p_.view(B, 32, 4, 32), v_.view(B, 32, 4, 32)).reshape(B, 128, 32)
            ctx = _f32(ctx + e3(ph, vl) + e3(pl_, vh) + e3(ph, vh))
        pm.append(_f32(m * _f32(torch.tensor(1.0 / LOG2E32, dtype=torch.float64))))
        pl.append(ls)
        pc.append(_f32(ga.view(B, 1, 1) * ctx + _f32(shv * ls.view(B, 128, 1))))
    return combine(torch.stack(pm, 1), torch.stack(pl, 1), torch.stack(pc, 1)).view(B, 4, 32, 32)


def x3_out_walk(c, ctx=None, defect=None):
    """attn_x3_fold and pass 2 (attn_x3_qz / attn_x3_z, which differ in where q~ comes from, not in a rounding) with every fp32 rounding point:
    the q projection in three terms, the softmax over d, q~ = e * (scale / sum) split into hi / lo, M_b as a chain of 32 fmas split into
    hi / lo, Z = bias + the three products.  Tiles are independent: all pixels at once.  `defect`: one term left out.
    Returns (y fp32, the M_b planes [B][2][C][4][32] bf16)."""
    B, N, C = c.B, c.N, c.C
    ctx = c.want_ctx.double() if ctx is None else ctx.double()
    bf = lambda t: t.float().bfloat16().double()
    split = lambda t: (bf(t), bf(_f32(t - bf(t))))
    ga2 = _f32(c.a.view(B, 1, 1) * LOG2E32)
    gam = (c.a * c.mean).view(B, 1)
    lab = torch.nan_to_num(_label(c), nan=0.0)
    shq = _f32(_f32(_f32(c.t1[:128].view(1, 128) - _f32(gam * c.t2[:128].view(1, 128))) + lab) * LOG2E32)
    xh, xl = split(c.x)
    wh, wl = split(c.wpk[:128])
    aq = _f32(xh @ wh.T + xh @ wl.T + (0.0 if defect == "x_lo_w_hi_dropped" else xl @ wh.T))
    q = _f32(ga2 * aq + shq.view(B, 1, 128)).view(B, N, 4, 32)
    e = _exp2_hw(_f32(q - q.amax(3, keepdim=True)))
    qt = _f32(e * _f32(c.scale / _f32(e.sum(3, keepdim=True))))
    qh, ql = split(qt)
    mb = torch.zeros(B, C, 4, 32, dtype=torch.float64)
    wo = c.wout.view(C, 4, 32)
    for e_ in range(32):                                     # acc = fmaf(w[e], ctx[d][e], acc), e ascending
        mb = _f32(mb + wo[:, :, e_].view(1, C, 4, 1) * ctx[:, :, :, e_].view(B, 1, 4, 32))
    mh, ml = split(mb)
    if defect == "mb_lo_dropped":
        ml = torch.zeros_like(ml)
    if defect == "q_lo_dropped":
        ql = torch.zeros_like(ql)
    z = _f32(c.bias.view(1, 1, C) + torch.einsum("bchd,bnhd->bnc", ml, qh) + torch.einsum("bchd,bnhd->bnc", mh, ql) + torch.einsum("bchd,bnhd->bnc", mh, qh))
    return z.float(), torch.stack([mh.float().bfloat16(), ml.float().bfloat16()], 1)


def _x(C, B, N, nseg, flavour="wlo", hint=0, label=True, gn="ab"):
    return dict(C=C, B=B, N=N, nseg=nseg, flavour=flavour, hint=hint, label=label, gn=gn)


def x3_gpu_cases():
    cs = []
    for C in (96, 192, 384):
        cs += [_x(C, 1, 1, 1, "small"), _x(C, 2, 33, 2, "wlo"), _x(C, 3, 65, 3, "qlo"), _x(C, 1, 129, 8, "wlo", gn="part"), _x(C, 2, 257, "lib", "small"),
               _x(C, 1, 257, 65, "qlo"), _x(C, 1, 1056, 3, "small", hint=256), _x(C, 1, 1057, "lib", "wlo", hint=512), _x(C, 2, 129, 2, "small", label=False, gn="part")]
    return cs


def x3_case_id(k):
    return "x3_C%d_B%d_N%d_s%s_h%d_%s%s_%s" % (k["C"], k["B"], k["N"], k["nseg"], k["hint"], k["flavour"], "" if k["label"] else "_nolabel", k["gn"])


def x3_resolve_nseg(k):
    return x3_segments(fused_batch(k["B"], k["hint"]), k["N"], k["C"]) if k["nseg"] == "lib" else k["nseg"]


_X3 = {}


def x3_build(k):
    key = (k["C"], k["B"], k["N"], k["flavour"], k["label"])
    if key not in _X3:
        _X3[key] = x3_case(k["C"], k["B"], k["N"], k["flavour"], k["label"])
    return _X3[key]
