"""Plain CPU helpers of tests/test_hip_linattn_paths.py and tests/test_linattn_ref_cpu.py: the two plain linear-attention files,
csrc/linattn.hip (ds_linattn_context / ds_linattn_output: attn_ctx_partial, attn_ctx_combine, attn_out_kernel) and csrc/vq_attn.hip
(ds_vq_attn_context / ds_vq_attn_output: vq_attn_ctx, vq_attn_fold, vq_attn_apply).  Layout as in tests/support_ref.py:

  launch arithmetic  the segment / block / group / tile ranges of a launch in plain Python, and the path predicates built on them ("this case
                     has an empty segment", "this block walks three groups"): the GPU test picks its shapes by them and asserts them;
  case builders      every input of a GPU test, the preconditions asserted BEFORE anything is launched;
  references         the operation in float64, rounded to bf16 exactly where the kernels store bf16 (wfold, the vq y, the bf16 linattn out);
  restatements       the kernels' own segment / tile order in torch fp32: on exact data they must give the reference's bits (the proof that
                     the data is exact), on random data they are the yardstick of the measured rule;
  defect models      what a kernel with one named fault would produce (the same walk with one hook).

Why the exact cases are exact.  Keys take the values 0, -200 and -400 only.  expf(0) = 1, and expf(-200), expf(-400), exp2(-288.5..) are 0
in fp32 (e^-200 = 1.4e-87 lies far below the smallest denormal), so every softmax weight over the pixels is 0 or 1: a hard selection of the
pixels whose key is 0.  A segment, tile or wave none of whose keys at d is 0 works under a local maximum of -200 or -400 and gives its
pixels weights of (about) 1 - and is wiped out exactly when it meets the true maximum: the online rescale multiplies it by
exp2(-288.5 - 0) = 0, the combine by expf(-200 - 0) = 0.  That needs one key equal to 0 per (sample, head, d) (or the extra token's key),
which the builders assert.  With integer v the context sums are integers below 2^24, the number of selected pixels (token included) is a
power of two, so A / L is exact; everything behind it (fold, output product, statistics) is a chain of fp32 fused multiply-adds on dyadic
numbers whose sum of magnitudes stays below 2^24 units: exact in any order.  The q softmax of attn_out_kernel gets the same treatment:
q + label_q in {0, -200, -400}, a power-of-two number of zeros per (pixel, head), scale = 0.25."""
import functools
import types

import torch

import exact_ref as E
from diffusynth_amd.synth import synth_input
from support_ref import NAN, _seed, check_guards, nan_slab, sig_bits, slab  # noqa: F401  (slab, nan_slab, check_guards: re-exported)

KEYS = (0.0, -200.0, -400.0)
PARTF = 32 + 32 + 1024
TP = 64                                      # pixels per sweep-2 tile of attn_ctx_partial
GP = 128                                     # pixels per group of the vq kernels: one 32-pixel tile per wave


def dyadic_unit(*ts):
    """The largest power of two u <= 1 of which every element of every tensor is a multiple."""
    u = 1.0
    for t in ts:
        t = t.double()
        while not torch.equal(t / u, (t / u).round()):
            u /= 2
            assert u >= 2.0 ** -40, "not dyadic"
    return u


def is_pow2(n):
    n = torch.as_tensor(n).to(torch.int64)
    return bool(((n > 0) & ((n & (n - 1)) == 0)).all())


# ================================================================================================= launch arithmetic (plain Python)
def rows_per_trip(bf16):
    """Rows one sweep-1 load of attn_ctx_partial<T> covers: 256 threads / (32 channels / (16 bytes / sizeof(T))) vectors."""
    return 256 // (32 // (16 // (2 if bf16 else 4)))


def segments(N, nseg):
    """[(n0, n1)] of attn_ctx_partial: per = ceil(N / nseg); n0 >= n1 is an empty segment."""
    per = (N + nseg - 1) // nseg
    return [(s * per, min(N, s * per + per)) for s in range(nseg)]


def seg_paths(N, nseg, bf16):
    """The paths of one ds_linattn_context launch, as a set of names."""
    R = rows_per_trip(bf16)
    out = set()
    segs = segments(N, nseg)
    lens = [max(0, n1 - n0) for n0, n1 in segs]
    for ln in lens:
        if ln == 0:
            out.add("empty_segment")
            continue
        out.add("len%d" % ln)
        if ln < R:
            out.add("shorter_than_a_load")
        if ln % (4 * R):
            out.add("clamped_trip")
        if ln > 4 * R:
            out.add("two_trips")
        if ln % TP:
            out.add("ragged_tile")
        if ln > TP:
            out.add("two_tiles")
    live = [ln for ln in lens if ln]
    if len(set(live)) > 1:
        out.add("ragged_last_segment")
    if nseg > 32:
        out.add("combine_second_batch")
    if nseg % 32:
        out.add("combine_ragged_batch")
    if nseg > 64:
        out.add("combine_third_batch")
    return out


def out_paths(N, bf16):
    """The paths of one ds_linattn_output launch."""
    out = set()
    blocks = (N + 255) // 256
    if blocks > 1:
        out.add("two_blocks")
    if blocks > 2:
        out.add("three_blocks")
    if N % 256:
        out.add("ragged_block")
    last = N - (blocks - 1) * 256                     # rows of the last block
    if not bf16:
        waves_in = (last + 63) // 64
        if waves_in < 4:
            out.add("wave_without_a_row")             # the fp32 row-transposition path: a wave all of whose 64 rows are clamped
        if last % 64:
            out.add("ragged_wave")
    return out


def vq_segments_rule(B, N, C):
    """ds_vq_attn_segments restated: min(64, (512 or 256) / B, ngroups) blocks, at least one, four partials each."""
    ngroups = (N + GP - 1) // GP
    return 4 * max(1, min(64, (512 if C <= 80 else 256) // max(B, 1), ngroups))


def vq_blocks(N, nseg):
    """(ngroups, [(g0, g1)] per block) of the vq kernels: nblk = nseg / 4, per = ceil(ngroups / nblk); g0 >= g1 is an empty block."""
    assert nseg >= 4 and nseg % 4 == 0
    ngroups, nblk = (N + GP - 1) // GP, nseg // 4
    per = (ngroups + nblk - 1) // nblk
    return ngroups, [(b * per, min(ngroups, b * per + per)) for b in range(nblk)]


def vq_block_pixels(N, nseg):
    """[(first pixel, one past the last)] per block: the pixels whose y the block stores and counts in its statistics slot."""
    return [(min(N, g0 * GP), min(N, max(g0, g1) * GP)) for g0, g1 in vq_blocks(N, nseg)[1]]


def vq_paths(N, nseg):
    out = set()
    ngroups, blocks = vq_blocks(N, nseg)
    for g0, g1 in blocks:
        if g0 >= g1:
            out.add("empty_block")
            continue
        out.add("walks%d" % (g1 - g0))
        if g1 - g0 >= 3:
            out.add("walks_three_or_more")            # the steady state of the double buffer: both parities, the g + 2 < g1 clamp
        for g in range(g0, g1):
            for w in range(4):
                px0 = g * GP + w * 32
                if px0 >= N:
                    out.add("wave_past_N")
                elif px0 + 32 > N:
                    out.add("ragged_tile")
                    if g > g0:
                        out.add("ragged_tile_in_a_later_group")
    return out


# ================================================================================================= linattn: cases
def _rank_select(score, count):
    """Boolean mask of the `count` smallest scores along the last dimension (count broadcasts over the leading ones)."""
    rank = score.argsort(-1).argsort(-1)
    return rank < count.unsqueeze(-1)


@functools.lru_cache(maxsize=None)
def linattn_case(bf16, B, N, heads, nseg, token=False, pad=0, q_softmax=0, lq=False, dead=()):
    """One exact ds_linattn_context + ds_linattn_output call.  token: the extra key / value of linear_cat; pad: the label strides are
    heads * 32 + pad with NaN in the gap; lq: label_q given (q_softmax = 1 only); dead: segments none of whose keys is 0.
    Fields (float64): q, k, v [B][N][heads][32], lk, lv, lqv [B][heads][32] or None, the *_full label buffers [B][stride], ctx [B][heads][32][32]
    = the exact context, out [B][N][heads * 32] = the exact output, want_ctx / want_out = what the kernels store."""
    HD = heads * 32
    g = E.gen(_seed("linattn", bf16, B, N, heads, nseg, token, pad, q_softmax, lq, dead))
    segs = segments(N, nseg)
    live = torch.ones(N, dtype=torch.bool)
    for s in dead:
        live[segs[s][0]:segs[s][1]] = False
    assert live.any()
    n_live = int(live.sum())
    # ---- token
    lk = lv = None
    tokzero = torch.zeros(B, heads, 32, dtype=torch.bool)
    if token:
        lk = E.choice(g, (B, heads, 32), [0.0, -200.0])
        lk[:, :, 0], lk[:, :, 1] = 0.0, -200.0
        lv = E.ints(g, (B, heads, 32), -100, 100)
        tokzero = lk == 0
    # ---- keys: per (b, h, d) a power-of-two number of selected keys (the token's among them); d = 0 with a token: the token alone
    # (every pixel key <= -200: the context row is lv); d = 2: the segment edges first (last row of every live segment, pixel 0)
    top = 1
    while 2 * top <= min(n_live, 64):
        top *= 2
    exps = torch.randint(0, top.bit_length(), (B, heads, 32), generator=g)
    total = 2 ** exps
    total[:, :, 2] = top
    if token:
        total[:, :, 0] = 1
    count = total - tokzero.long()
    score = torch.rand(B, heads, 32, N, generator=g)
    score[..., ~live] = 2.0 + score[..., ~live]
    edges = sorted({n1 - 1 for s, (n0, n1) in enumerate(segs) if n1 > n0 and s not in dead} | ({0} if live[0] else set()))
    prio = [N - 1] if live[N - 1] else []
    prio += [e for e in edges if e not in prio]
    for i, e in enumerate(prio):
        score[:, :, 2, e] = -1.0 + i * 1e-4
    sel = _rank_select(score, count)                                             # [B][heads][32][N]
    assert not sel[..., ~live].any()
    k = torch.where(sel, torch.zeros(()).double(), E.choice(g, sel.shape, [-200.0, -400.0])).permute(0, 3, 1, 2).contiguous()
    v = E.ints(g, (B, N, heads, 32), -100, 100)
    # ---- q
    scale = 0.25 if q_softmax else 1.0
    lqv = None
    if q_softmax:
        zset = torch.ones(B, heads, 32, dtype=torch.bool)
        if lq:
            zset = _rank_select(torch.rand(B, heads, 32, generator=g), torch.full((B, heads), 24))
            lqv = torch.where(zset, 0.0, -200.0).double()
        qexp = torch.randint(0, 5, (B, N, heads), generator=g)
        qs = torch.rand(B, N, heads, 32, generator=g) + (~zset).double().unsqueeze(1) * 2.0
        qsel = _rank_select(qs, 2 ** qexp)
        q = torch.where(qsel, 0.0, -200.0).double()
        q = torch.where(zset.unsqueeze(1) | (torch.rand(q.shape, generator=g) < 0.5), q, torch.zeros(()).double())   # off the label's zeros: 0 too
    else:
        assert not lq
        q = E.ints(g, (B, N, heads, 32), -8, 8)
    c = types.SimpleNamespace(bf16=bool(bf16), B=B, N=N, heads=heads, HD=HD, nseg=nseg, token=token, pad=pad, q_softmax=q_softmax, scale=scale,
                              dead=tuple(dead), q=q, k=k, v=v, lk=lk, lv=lv, lqv=lqv, stride=HD + pad,
                              id="%s_B%d_N%d_h%d_s%d%s%s%s%s%s" % ("bf16" if bf16 else "f32", B, N, heads, nseg, "_tok" if token else "", "_pad%d" % pad if pad else "",
                                                                   "_qs" if q_softmax else "", "_lq" if lq else "", "_dead%s" % "-".join(map(str, dead)) if dead else ""))
    for name in ("lk", "lv", "lqv"):
        t = getattr(c, name)
        full = None
        if t is not None:
            full = torch.full((B, HD + pad), NAN, dtype=torch.float64)
            full[:, :HD] = t.reshape(B, HD)
        setattr(c, name + "_full", full)
    linattn_preconditions(c)
    return c


def linattn_qkv(c):
    """[B][N][3 * heads * 32] of the kernel's dtype: q | k | v, each (head, d)."""
    t = torch.cat([c.q.reshape(c.B, c.N, c.HD), c.k.reshape(c.B, c.N, c.HD), c.v.reshape(c.B, c.N, c.HD)], -1)
    return t.float().bfloat16() if c.bf16 else t.float()


def linattn_preconditions(c):
    """Key alphabet, a zero key per (b, h, d), power-of-two counts, sum |.| < 2^24 at every intermediate; sets c.ctx, c.out, c.want_*."""
    B, N, H = c.B, c.N, c.heads
    for t in (c.q, c.k, c.v):
        assert E.is_bf16(t) if c.bf16 else E.is_f32(t)
    assert bool(torch.isin(c.k, torch.tensor(KEYS, dtype=torch.float64)).all())
    zeros = (c.k == 0).sum(1)                                                    # [B][H][32]
    if c.token:
        assert bool(torch.isin(c.lk, torch.tensor(KEYS, dtype=torch.float64)).all()) and E.is_f32(c.lv)
        zeros = zeros + (c.lk == 0).long()
        assert bool(((c.k == 0).sum(1)[:, :, 0] == 0).all()) and bool((c.lk[:, :, 0] == 0).all()), "d = 0: the token dominates"
        assert bool((c.lk[:, :, 1] == -200).all()), "d = 1: the token is negligible"
    assert is_pow2(zeros), "the selected keys per (b, h, d) must number a power of two (and at least one)"
    segs = segments(N, c.nseg)
    for s in c.dead:
        n0, n1 = segs[s]
        assert n1 > n0 and bool((c.k[:, n0:n1] <= -200).all()), "segment %d was to have no zero key" % s
    sel = (c.k == 0).double()
    A = torch.einsum("bnhd,bnhe->bhde", sel, c.v)
    assert c.v.abs().sum(1).max().item() < E.LIMIT                               # every partial context sum, selected or not
    if c.token:
        A = A + (c.lk == 0).double().unsqueeze(-1) * c.lv.unsqueeze(2)
    c.ctx = A / zeros.double().unsqueeze(-1)
    assert E.is_f32(c.ctx)
    if c.token:
        assert torch.equal(c.ctx[:, :, 0], c.lv), "the context row of a dominating token is lv"
    c.counts = zeros
    # ---- output
    if c.q_softmax:
        qq = c.q + (c.lqv.unsqueeze(1) if c.lqv is not None else 0.0)
        assert bool(torch.isin(qq, torch.tensor(KEYS, dtype=torch.float64)).all())
        qz = (qq == 0).sum(-1)
        assert is_pow2(qz), "the zeros of q + label_q per (pixel, head) must number a power of two"
        qt = (qq == 0).double() / qz.double().unsqueeze(-1) * c.scale
    else:
        qt = c.q
    unit = dyadic_unit(c.ctx) * dyadic_unit(qt)
    c.out_margin = torch.einsum("bhde,bnhd->bnhe", c.ctx.abs(), qt.abs()).max().item() / unit
    E.check_exact(c.out_margin)
    c.qt = qt
    c.out = torch.einsum("bhde,bnhd->bnhe", c.ctx, qt).reshape(B, N, c.HD)
    assert E.is_f32(c.out)
    c.want_ctx = c.ctx.float()
    c.want_out = E.store(c.out, c.bf16)
    if c.bf16 and c.out.numel() >= 4096:
        assert E.rounding_profile(c.out)[0] >= 0.05, "the bf16 store of out was to round"
    return c


def linattn_ref64(c):
    """(ctx, out) by the formula of include/diffusynth_hip.h in float64, softmax and all: independent of the selection argument above.
    ctx is rounded to fp32 where the kernel stores it (pass 2 reads the stored context)."""
    k, v = c.k.permute(0, 2, 3, 1), c.v.permute(0, 2, 3, 1)                      # [B][H][32][N]
    if c.token:
        k = torch.cat([k, c.lk.unsqueeze(-1)], -1)
        v = torch.cat([v, c.lv.unsqueeze(-1)], -1)
    ctx = torch.einsum("bhdn,bhen->bhde", k.softmax(-1), v).float()
    q = c.q
    if c.q_softmax:
        q = (q + (c.lqv.unsqueeze(1) if c.lqv is not None else 0.0)).softmax(-1) * c.scale
    out = torch.einsum("bhde,bnhd->bnhe", ctx.double(), q).reshape(c.B, c.N, c.HD)
    return ctx, out


# ------------------------------------------------------------------------------------------------- linattn: the kernels' walk
LINATTN_MUTANTS = ("seg_last_row_dropped", "tile_clamp_counted", "sweep1_trip_clamp_wrong_max", "combine_second_batch_lost",
                   "combine_ragged_batch_counted_twice", "token_ignored", "token_stride_as_HD", "lq_stride_as_HD", "k_v_offsets_swapped",
                   "head_h_reads_head_0", "out_second_block_lost", "empty_segment_counted")


def _combine(ms, ls, cs, lk, lv, fault=None):
    """attn_ctx_combine: ms, ls [S][...][32], cs [S][...][32][32]; the token (lk, lv [...][32]) or None; batches of 32 segments in ascending
    order, the entries of a ragged batch clamped to the last segment and weighted 0."""
    S = ms.shape[0]
    M = ms.max(0).values
    if lk is not None:
        M = torch.maximum(M, lk)
        w = torch.exp(lk - M)
        Lr, A = w.clone(), w.unsqueeze(-1) * lv.unsqueeze(-2)
    else:
        Lr, A = torch.zeros_like(M), torch.zeros_like(cs[0])
    for s0 in range(0, S, 32):
        if fault == "combine_second_batch_lost" and s0 >= 32:
            break
        nb = min(32, S - s0)
        for j in range(32):
            if j >= nb and fault != "combine_ragged_batch_counted_twice":
                continue                                                        # (f = 0 times a finite partial)
            s = min(s0 + j, S - 1)
            f = torch.exp(ms[s] - M)
            Lr = Lr + f * ls[s]
            A = A + f.unsqueeze(-1) * cs[s]
    return A / Lr.unsqueeze(-1)


def _labels(full, B, HD, stride, as_hd):
    """[B][HD] read from a [B][stride] label buffer; as_hd: the fault of a kernel that strides by heads * 32."""
    if not as_hd:
        return full[:, :HD]
    flat = full.flatten()
    return torch.stack([flat[b * HD:(b + 1) * HD] for b in range(B)])


def linattn_ctx_walk(c, nseg=None, fault=None, dtype=torch.float32):
    """ds_linattn_context segment by segment in `dtype` (fp32: the restatement; with `fault`: a defect model): per segment the maximum,
    exp(k - max), its row sums and P^T V; then _combine.  Returns ctx [B][heads][32][32]."""
    B, N, H = c.B, c.N, c.heads
    nseg = c.nseg if nseg is None else nseg
    R = rows_per_trip(c.bf16)
    k, v = c.k.to(dtype), c.v.to(dtype)
    if fault == "k_v_offsets_swapped":
        k, v = v, k
    if fault == "head_h_reads_head_0":
        k, v = k[:, :, :1].expand_as(k), v[:, :, :1].expand_as(v)
    ms, ls, cs = [], [], []
    for n0, n1 in segments(N, nseg):
        if fault == "seg_last_row_dropped":
            n1 = max(n0, n1 - 1)
        rows = list(range(n0, n1))
        if not rows and fault == "empty_segment_counted":
            rows = [N - 1]                                                       # the clamped row of a kernel that loads without looking
        if not rows:
            ms.append(torch.full((B, H, 32), -float("inf"), dtype=dtype))
            ls.append(torch.zeros(B, H, 32, dtype=dtype))
            cs.append(torch.zeros(B, H, 32, 32, dtype=dtype))
            continue
        rows_max, rows_sum = rows, rows
        if fault == "sweep1_trip_clamp_wrong_max":
            rows_max = rows[:len(rows) // (4 * R) * (4 * R)] + [rows[-1]]         # an incomplete trip sees its clamp row only
        if fault == "tile_clamp_counted":
            rows_sum = rows + [rows[-1]] * ((-len(rows)) % TP)                   # the clamped rows of the last tile not zeroed
        m = k[:, rows_max].max(1).values
        P = torch.exp(k[:, rows_sum] - m.unsqueeze(1))
        ms.append(m)
        ls.append(P.sum(1))
        cs.append(torch.einsum("bnhd,bnhe->bhde", P, v[:, rows_sum]))
    lk = lv = None
    if c.token and fault != "token_ignored":
        as_hd = fault == "token_stride_as_HD"
        lk = _labels(c.lk_full, B, c.HD, c.stride, as_hd).reshape(B, H, 32).to(dtype)
        lv = _labels(c.lv_full, B, c.HD, c.stride, as_hd).reshape(B, H, 32).to(dtype)
    return _combine(torch.stack(ms), torch.stack(ls), torch.stack(cs), lk, lv, fault)


def linattn_out_walk(c, ctx, fault=None, dtype=torch.float32, prefill=NAN):
    """ds_linattn_output in `dtype` on a given context: the softmax over d as the kernel computes it (maximum, exp, sum, one reciprocal,
    times scale), the product with the context.  [B][N][heads * 32], not yet rounded to the output type."""
    B, N, H = c.B, c.N, c.heads
    q = c.q.to(dtype)
    if c.q_softmax:
        if c.lqv is not None:
            q = q + _labels(c.lqv_full, B, c.HD, c.stride, fault == "lq_stride_as_HD").reshape(B, 1, H, 32).to(dtype)
        e = torch.exp(q - q.max(-1, keepdim=True).values)
        q = e * (1.0 / e.sum(-1, keepdim=True)) * torch.tensor(c.scale, dtype=dtype)
    out = torch.einsum("bhde,bnhd->bnhe", ctx.to(dtype), q).reshape(B, N, c.HD)
    if fault == "out_second_block_lost":
        out = out.clone()
        out[:, 256:] = prefill
    return out


def linattn_mutant(c, kind):
    """(ctx, out) as fp32 / the output type, of a kernel pair with one fault, or None where the fault cannot show in this case."""
    segs = segments(c.N, c.nseg)
    lens = [max(0, n1 - n0) for n0, n1 in segs]
    need = {"tile_clamp_counted": any(ln % TP for ln in lens if ln), "sweep1_trip_clamp_wrong_max": any(ln % (4 * rows_per_trip(c.bf16)) for ln in lens if ln),
            "combine_second_batch_lost": c.nseg > 32, "combine_ragged_batch_counted_twice": c.nseg % 32 != 0, "token_ignored": c.token,
            "token_stride_as_HD": c.token and c.pad > 0 and c.B > 1, "lq_stride_as_HD": c.lqv is not None and c.pad > 0 and c.B > 1,
            "head_h_reads_head_0": c.heads > 1, "out_second_block_lost": c.N > 256, "empty_segment_counted": 0 in lens}
    if not need.get(kind, True):
        return None
    assert kind in LINATTN_MUTANTS, kind
    ctx = linattn_ctx_walk(c, fault=kind)
    out = linattn_out_walk(c, c.want_ctx if kind in ("lq_stride_as_HD", "out_second_block_lost") else ctx, fault=kind)
    return ctx, (out.bfloat16() if c.bf16 else out)


@functools.lru_cache(maxsize=None)
def linattn_random_case(bf16, B, N, heads, nseg, kind):
    """Random data, the model's scale 32 ** -0.5: kind in add (label_q), cat (the token, strides padded), vqgan (raw q), spike (two keys far
    above the rest: the cross-segment rescale with generic weights).  The inputs are rounded to the kernel's dtype first."""
    tag = "linattn_paths:%s:%d:%d:%d:%s" % (bf16, B, N, heads, kind)
    HD = heads * 32
    rnd = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.float().double())
    qkv = synth_input(tag, (B, N, 3, heads, 32)) * 2.0
    if kind == "spike":
        qkv[:, N // 3, 1, 0, 3] += 30.0
        qkv[:, N - 1, 1, heads - 1, 8] += 45.0
    qkv = rnd(qkv)
    pad = 8 if kind == "cat" else 0
    c = types.SimpleNamespace(bf16=bool(bf16), B=B, N=N, heads=heads, HD=HD, nseg=nseg, token=kind == "cat", pad=pad, stride=HD + pad,
                              q_softmax=int(kind != "vqgan"), scale=32 ** -0.5 if kind != "vqgan" else 1.0, q=qkv[:, :, 0], k=qkv[:, :, 1], v=qkv[:, :, 2],
                              lk=None, lv=None, lqv=None, id="%s_%s_B%d_N%d_h%d_s%d" % ("bf16" if bf16 else "f32", kind, B, N, heads, nseg))
    if kind in ("add", "spike"):
        c.lqv = synth_input(tag + ":lq", (B, heads, 32)).double()
    if kind == "cat":
        c.lk, c.lv = synth_input(tag + ":lk", (B, heads, 32)).double() * 3, synth_input(tag + ":lv", (B, heads, 32)).double()
    for name in ("lk", "lv", "lqv"):
        t, full = getattr(c, name), None
        if t is not None:
            full = torch.full((B, HD + pad), NAN, dtype=torch.float64)
            full[:, :HD] = t.reshape(B, HD)
        setattr(c, name + "_full", full)
    return c


def row_errors(got, want):
    """Per row (last dimension) max |got - want| / max |want|: [rows] float64.  The error of a row is scaled by the row's OWN L-infinity norm,
    so that a fault confined to one pixel row is as large as it would be in a tensor of that one row."""
    got, want = got.double().reshape(-1, got.shape[-1]), want.double().reshape(-1, want.shape[-1])
    return (got - want).abs().max(1).values / want.abs().max(1).values.clamp_min(1e-30)


# ================================================================================================= vq_attn: cases
NSEL, NWIDE = 8, 16                          # selector channels [0, 8): x in {0, 1, 2}, k = -200 x;  wide channels [8, 24): x in {0, +-128}
VQ_MUTANTS = ("ragged_rows_unmasked", "wave_past_N_counted", "group_parity_swapped", "third_group_stale", "empty_block_stats_stale", "wnin_dropped",
              "bias_dropped", "fold_rows_past_C_kept", "ctx_transposed")


@functools.lru_cache(maxsize=None)
def vq_case(C, B, N, skip=True):
    """One exact data set for ds_vq_attn_context / ds_vq_attn_output (every nseg runs on the same data; vq_expect gives what a launch with
    a given nseg stores).  Channels of x: NSEL selectors valued {0, 1, 2} (Wk has one -200 per d on them and nothing else, so k = Wk x is 0,
    -200 or -400), NWIDE wide channels (at most one per pixel, +-128: only Wnin reads them, with weights +-n / 512, 513 <= n < 576, that
    need ten significant bits - the bf16 store of the fold rounds them to a multiple of 1 / 128 and their product with x stays an integer),
    the others small integers that drive v (Wv: one +-16 per e) and q (Wq: one +-1 per d)."""
    g = E.gen(_seed("vq_attn", C, B, N, skip))
    V0 = NSEL + NWIDE
    NV = C - V0
    x = torch.zeros(B, N, C, dtype=torch.float64)
    # selectors: a power-of-two number of zeros per (sample, selector), at most 16
    top = 1
    while 2 * top <= min(N, 16):
        top *= 2
    cnt = 2 ** torch.randint(0, top.bit_length(), (B, NSEL), generator=g)
    cnt[:, 0] = top
    score = torch.rand(B, NSEL, N, generator=g)
    score[:, 0, N - 1] = -1.0                                                    # the last pixel (of a ragged tile) is selected somewhere
    zero = _rank_select(score, cnt)                                              # [B][NSEL][N]
    x[:, :, :NSEL] = torch.where(zero, torch.zeros(()).double(), E.choice(g, zero.shape, [1.0, 2.0])).permute(0, 2, 1)
    # wide: a quarter of the pixels carry one
    wch = torch.randint(0, NWIDE, (B, N), generator=g)
    won = torch.rand(B, N, generator=g) < 0.25
    wval = E.choice(g, (B, N), [-128.0, 128.0]) * won
    x[:, :, NSEL:V0].scatter_(2, wch.unsqueeze(-1), wval.unsqueeze(-1))
    # values: four channels of +-1 per pixel
    vsel = _rank_select(torch.rand(B, N, NV, generator=g), torch.full((B, N), 4))
    x[:, :, V0:] = E.choice(g, (B, N, NV), [-1.0, 1.0]) * vsel
    wqkv = torch.zeros(96, C, dtype=torch.float64)
    d = torch.arange(32)
    wqkv[32 + d, d % NSEL] = -200.0
    wqkv[64 + d, V0 + torch.randint(0, NV, (32,), generator=g)] = E.choice(g, (32,), [-16.0, 16.0])
    wqkv[d, V0 + torch.randint(0, NV, (32,), generator=g)] = E.choice(g, (32,), [-1.0, 1.0])
    wout = torch.zeros(C, 32, dtype=torch.float64)
    wout[torch.arange(C), torch.randint(0, 32, (C,), generator=g)] = E.choice(g, (C,), [-1.0, 1.0])
    bias = E.ints(g, (C,), -3, 3)
    wnin = None
    if skip:
        wnin = torch.zeros(C, C, dtype=torch.float64)
        wnin[:, V0:] = E.ints(g, (C, NV), -1, 1, density=0.25)
        wnin[:, NSEL:V0] = E.ints(g, (C, NWIDE), 513, 575) / 512.0 * E.choice(g, (C, NWIDE), [-1.0, 1.0])
    c = types.SimpleNamespace(C=C, CP=(C + 31) // 32 * 32, B=B, N=N, skip=skip, x=x, wqkv=wqkv, wq=wqkv[:32].clone(), wout=wout, wnin=wnin, bias=bias,
                              id="C%d_B%d_N%d%s" % (C, B, N, "" if skip else "_noskip"))
    vq_preconditions(c)
    return c


def vq_preconditions(c):
    """The key alphabet, a zero key per (b, d) in a power-of-two number, and sum |.| < 2^24 units at k, v, the context sums, T = ctx Wq, W_b and
    y; |y| <= 256 and integer (its bf16 store does not round); a share of W_b needs more than 8 significant bits (its bf16 store does).
    Sets c.ctx, c.wb (before the store), c.wfold [B][CP][C] and c.y [B][N][C] (as stored, float64)."""
    B, N, C = c.B, c.N, c.C
    assert E.is_bf16(c.x) and E.is_bf16(c.wqkv) and E.is_f32(c.wout) and E.is_f32(c.bias) and (c.wnin is None or E.is_f32(c.wnin))
    wk, wv = c.wqkv[32:64], c.wqkv[64:]
    k, v = c.x @ wk.T, c.x @ wv.T                                                # [B][N][32]
    E.check_exact((c.x.abs() @ wk.abs().T).max().item())
    E.check_exact((c.x.abs() @ wv.abs().T).max().item())
    assert bool(torch.isin(k, torch.tensor(KEYS, dtype=torch.float64)).all()), "k = Wk x must be 0, -200 or -400"
    zeros = (k == 0).sum(1)                                                      # [B][32]
    assert is_pow2(zeros), "the zero keys per (b, d) must number a power of two (and at least one)"
    assert E.is_bf16(v) and v.abs().max().item() <= 256, "v enters the matrix cores as bf16"
    assert v.abs().sum(1).max().item() < E.LIMIT
    c.k, c.v, c.counts = k, v, zeros
    c.ctx = torch.einsum("bnd,bne->bde", (k == 0).double(), v) / zeros.double().unsqueeze(-1)
    assert E.is_f32(c.ctx)
    T = torch.einsum("bde,dc->bec", c.ctx, c.wq)
    u = dyadic_unit(c.ctx) * dyadic_unit(c.wq)
    E.check_exact(torch.einsum("bde,dc->bec", c.ctx.abs(), c.wq.abs()).max().item() / u)
    wb = torch.einsum("oe,bec->boc", c.wout, T)
    mag = torch.einsum("oe,bec->boc", c.wout.abs(), torch.einsum("bde,dc->bec", c.ctx.abs(), c.wq.abs()))
    if c.wnin is not None:
        wb, mag = wb + c.wnin, mag + c.wnin.abs()
    u = dyadic_unit(wb, T) * dyadic_unit(c.wout)
    E.check_exact(mag.max().item() / u)
    assert E.is_f32(wb)
    c.T, c.wb = T, wb
    c.wide_share = (sig_bits(wb / dyadic_unit(wb)) > 8).double().mean().item()
    if c.wnin is not None:
        assert c.wide_share >= 0.05, "only %.3f of the W_b entries need more than 8 significant bits" % c.wide_share
        assert E.rounding_profile(wb)[1] > 0, "no exact tie among the W_b entries"
    c.wfold = torch.zeros(B, c.CP, C, dtype=torch.float64)
    c.wfold[:, :C] = E.rne_bf16(wb).double()
    y = torch.einsum("boc,bnc->bno", c.wfold[:, :C], c.x) + c.bias
    u = dyadic_unit(c.wfold) * dyadic_unit(c.x)
    c.y_margin = (torch.einsum("boc,bnc->bno", c.wfold[:, :C].abs(), c.x.abs()) + c.bias.abs()).max().item() / u
    E.check_exact(c.y_margin)
    assert torch.equal(y, y.round()) and y.abs().max().item() <= 256 and E.is_bf16(y), "|y| reaches %g" % y.abs().max().item()
    assert (y * y).sum(1).max().item() < E.LIMIT and y.abs().sum(1).max().item() < E.LIMIT, "the statistics of one block (at most the whole sample)"
    c.y = y
    return c


def vq_ref64(c):
    """(ctx fp32, wfold bf16 [B][CP][C], y bf16 [B][N][C]) by the header's formula in float64 (a true softmax over the pixels), rounded where the
    kernels store: ctx to fp32, W_b and y to bf16."""
    k, v = c.x @ c.wqkv[32:64].T, c.x @ c.wqkv[64:].T
    ctx = torch.einsum("bnd,bne->bde", k.softmax(1), v).float()
    wb = torch.einsum("oe,bec->boc", c.wout, torch.einsum("bde,dc->bec", ctx.double(), c.wq))
    if c.wnin is not None:
        wb = wb + c.wnin
    wfold = torch.zeros(c.B, c.CP, c.C, dtype=torch.bfloat16)
    wfold[:, :c.C] = E.rne_bf16(wb)
    y = torch.einsum("boc,bnc->bno", wfold[:, :c.C].double(), c.x) + c.bias
    return ctx, wfold, E.rne_bf16(y)


def vq_stats(y, N, nseg, fault=None):
    """[B][nseg / 4][C][2] float64: (sum, sum of squares) of the stored y over each block's pixels; an empty block's slot is 0."""
    B, _, C = y.shape
    out = torch.zeros(B, nseg // 4, C, 2, dtype=torch.float64)
    for i, (p0, p1) in enumerate(vq_block_pixels(N, nseg)):
        yy = y[:, p0:p1].double()
        out[:, i, :, 0], out[:, i, :, 1] = yy.sum(1), (yy * yy).sum(1)
        if p0 >= p1 and fault == "empty_block_stats_stale":
            out[:, i] = NAN
    return out


def _vq_group_source(N, nseg, fault):
    """Pixel -> the pixel whose x a faulty double buffer hands the kernel instead (-1: a zero row); identity without a fault."""
    src = torch.arange(N)
    for g0, g1 in vq_blocks(N, nseg)[1]:
        for i, g in enumerate(range(g0, g1)):
            gs = g
            if fault == "third_group_stale" and i >= 2:
                gs = g - 2
            if fault == "group_parity_swapped" and g0 + (i ^ 1) < g1:
                gs = g0 + (i ^ 1)
            p = torch.arange(g * GP, min(N, (g + 1) * GP))
            s = p + (gs - g) * GP
            src[p] = torch.where(s < N, s, torch.full_like(s, -1))
    return src


def _vq_x(c, N, nseg, fault, dtype):
    x = c.x.to(dtype)
    if fault in ("third_group_stale", "group_parity_swapped"):
        src = _vq_group_source(N, nseg, fault)
        x = torch.where((src >= 0).view(1, N, 1), x[:, src.clamp_min(0)], torch.zeros((), dtype=dtype))
    return x


def vq_ctx_walk(c, nseg, fault=None, dtype=torch.float32, round_pv=False):
    """ds_vq_attn_context block by block, wave by wave, tile by tile in `dtype`: the online softmax over the pixels with its rescale, one
    (max, sum, ctx) partial per wave, then _combine.  round_pv: P and V rounded to bf16 for the context product, as the matrix cores take
    them (the row sums keep the unrounded P): the restatement of the random-data cases."""
    B, N = c.B, c.N
    x = _vq_x(c, N, nseg, fault, dtype)
    k, v = x @ c.wqkv[32:64].to(dtype).T, x @ c.wqkv[64:].to(dtype).T
    pv = (lambda t: t.bfloat16().to(dtype)) if round_pv else (lambda t: t)
    ninf = -float("inf")
    ms, ls, cs = [], [], []
    for g0, g1 in vq_blocks(N, nseg)[1]:
        for w in range(4):
            m, l, ctx = torch.full((B, 32), ninf, dtype=dtype), torch.zeros(B, 32, dtype=dtype), torch.zeros(B, 32, 32, dtype=dtype)
            for g in range(g0, g1):
                px0 = g * GP + w * 32
                if px0 >= N and fault != "wave_past_N_counted":
                    continue
                kt, vt = torch.zeros(B, 32, 32, dtype=dtype), torch.zeros(B, 32, 32, dtype=dtype)       # rows past N: zero-filled x
                r = max(0, min(32, N - px0))
                kt[:, :r], vt[:, :r] = k[:, px0:px0 + r], v[:, px0:px0 + r]
                if fault not in ("ragged_rows_unmasked", "wave_past_N_counted") or (fault == "wave_past_N_counted" and r > 0):
                    kt[:, r:] = ninf
                mn = torch.maximum(m, kt.max(1).values)
                sc = torch.where(m == ninf, torch.zeros((), dtype=dtype), torch.exp(m - mn))
                P = torch.exp(kt - mn.unsqueeze(1))
                l = l * sc + P.sum(1)
                ctx = ctx * sc.unsqueeze(-1) + torch.einsum("brd,bre->bde", pv(P), pv(vt))
                m = mn
            ms.append(m)
            ls.append(l)
            cs.append(ctx)
    return _combine(torch.stack(ms), torch.stack(ls), torch.stack(cs), None, None)


def vq_out_walk(c, ctx, nseg, fault=None, dtype=torch.float32, prefill=NAN):
    """ds_vq_attn_output in `dtype` on a given context: (wfold [B][CP][C] bf16, y [B][N][C] bf16).  The fold as the kernel orders it
    (T = ctx Wq first, then Wnin + Wout T), one rounding to bf16; y = W_b x + bias, one rounding to bf16."""
    B, N, C = c.B, c.N, c.C
    cx = ctx.to(dtype)
    if fault == "ctx_transposed":
        cx = cx.transpose(1, 2)
    T = torch.einsum("bde,dc->bec", cx, c.wq.to(dtype))
    wb = torch.einsum("oe,bec->boc", c.wout.to(dtype), T)
    if c.wnin is not None and fault != "wnin_dropped":
        wb = c.wnin.to(dtype) + wb
    wfold = torch.full((B, c.CP, C), prefill if fault == "fold_rows_past_C_kept" else 0.0, dtype=torch.bfloat16)
    wfold[:, :C] = wb.float().bfloat16()
    y = torch.einsum("boc,bnc->bno", wfold[:, :C].to(dtype), _vq_x(c, N, nseg, fault, dtype))
    if fault != "bias_dropped":
        y = y + c.bias.to(dtype)
    return wfold, y.float().bfloat16()


def vq_expect(c, nseg):
    """What a launch pair with this nseg stores, from the float64 reference: ctx fp32, wfold bf16, y bf16, stats float64 [B][nseg / 4][C][2]."""
    ctx, wfold, y = vq_ref64(c)
    return types.SimpleNamespace(ctx=ctx, wfold=wfold, y=y, stats=vq_stats(y, c.N, nseg))


def vq_mutant(c, nseg, kind):
    """(ctx, wfold, y, stats) of a kernel chain with one fault, or None where the fault cannot show at this shape."""
    assert kind in VQ_MUTANTS, kind
    paths = vq_paths(c.N, nseg)
    need = {"ragged_rows_unmasked": "ragged_tile" in paths, "wave_past_N_counted": "wave_past_N" in paths, "group_parity_swapped": any(p in paths for p in ("walks2", "walks_three_or_more")),
            "third_group_stale": "walks_three_or_more" in paths, "empty_block_stats_stale": "empty_block" in paths, "wnin_dropped": c.wnin is not None,
            "fold_rows_past_C_kept": c.CP > c.C}
    if not need.get(kind, True):
        return None
    ctx = vq_ctx_walk(c, nseg, fault=kind)
    wfold, y = vq_out_walk(c, ctx, nseg, fault=kind)
    return ctx, wfold, y, vq_stats(y, c.N, nseg, fault=kind)


@functools.lru_cache(maxsize=None)
def vq_random_case(C, B, N, skip):
    """The data of tests/test_hip_tail.py::test_vq_attn_fused_matches_torch at a shape of this file: x and to_qkv rounded to bf16."""
    tag = "vq_paths:%d:%d:%d" % (C, B, N)
    wqkv = (synth_input(tag + ":wqkv", (96, C)) * (2.0 / C ** 0.5)).bfloat16().double()
    wq32 = (synth_input(tag + ":wqkv", (96, C)) * (2.0 / C ** 0.5))[:32].double()                  # the fold reads the fp32 to_qkv.weight
    return types.SimpleNamespace(C=C, CP=(C + 31) // 32 * 32, B=B, N=N, skip=skip, x=(synth_input(tag + ":x", (B, N, C)) * 1.3 + 0.1).bfloat16().double(),
                                 wqkv=wqkv, wq=wq32, wout=synth_input(tag + ":wo", (C, 32)).double() * 0.2,
                                 wnin=synth_input(tag + ":wn", (C, C)).double() * (1.0 / C ** 0.5) if skip else None,
                                 bias=synth_input(tag + ":b", (C,)).double() * 0.3, id="random_C%d_B%d_N%d%s" % (C, B, N, "" if skip else "_noskip"))


# ================================================================================================= the shapes of the GPU test
def _seg_lengths(bf16):
    R = rows_per_trip(bf16)
    return sorted({1, R - 1, R, R + 1, 63, 64, 65, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 1})


def linattn_partial_args():
    """attn_ctx_partial<T>: every segment length of the list as per = ceil(N / 2) with a ragged second segment (N = 2 per - 1; per = 1: N = 2),
    heads 1, 4, 8 and B 1, 3 in turn; the longest alone (nseg = 1); N = 10 in 7 segments (two empty)."""
    out = []
    for bf16 in (False, True):
        for i, per in enumerate(_seg_lengths(bf16)):
            N = 2 * per - 1 if per > 1 else 2
            if N > 700:
                N, ns = per, 1
            else:
                ns = 2
            out.append(dict(bf16=bf16, B=(1, 3)[i % 2], N=N, heads=(1, 4, 8)[i % 3], nseg=ns, token=i % 4 == 1, pad=8 if i % 4 == 1 else 0))
        out.append(dict(bf16=bf16, B=3, N=10, heads=4, nseg=7))
        out.append(dict(bf16=bf16, B=1, N=10, heads=1, nseg=7, token=True, pad=8))
    return out


def linattn_combine_args():
    """attn_ctx_combine through ds_linattn_context at N = 130: nseg 1, 31, 32, 33, 64, 65, a segment without a zero key in every batch of
    32, the token absent and present (dominating at d = 0, negligible at d = 1), label strides of heads * 32 + 8 with NaN in the gap."""
    out = []
    for i, ns in enumerate((1, 31, 32, 33, 64, 65)):
        per = (130 + ns - 1) // ns
        nlive = (130 + per - 1) // per
        dead = tuple(s for s in (1, 40) if s < nlive - 1)
        out.append(dict(bf16=bool(i % 2), B=3, N=130, heads=4, nseg=ns, token=True, pad=8, dead=dead))
        out.append(dict(bf16=not i % 2, B=1, N=130, heads=1, nseg=ns, dead=dead))
    return out


def linattn_output_args():
    """attn_out_kernel<T>: N of the list, heads 1, 4, 7, 8, q_softmax 0 and 1 (scale 0.25), label_q NULL and set with a padded stride."""
    out = []
    for bf16 in (False, True):
        for i, N in enumerate((1, 63, 64, 65, 255, 256, 257, 513)):
            h = (1, 4, 7, 8)[i % 4]
            out.append(dict(bf16=bf16, B=(3, 1)[i % 2], N=N, heads=h, nseg=min(N, 2), q_softmax=1, lq=True, pad=8))
            out.append(dict(bf16=bf16, B=(1, 3)[i % 2], N=N, heads=(8, 7, 4, 1)[i % 4], nseg=1, q_softmax=i % 2, lq=False))
    return out


def linattn_args():
    seen, out = set(), []
    for a in linattn_partial_args() + linattn_combine_args() + linattn_output_args():
        key = tuple(sorted(a.items()))
        if key not in seen:
            seen.add(key)
            out.append(a)
    return out


LINATTN_RANDOM = ((False, 3, 257, 4, 3, "add"), (False, 1, 130, 8, 33, "cat"), (False, 2, 65, 1, 2, "vqgan"), (False, 2, 513, 7, 5, "spike"),
                  (True, 3, 257, 4, 3, "add"), (True, 1, 130, 8, 33, "cat"), (True, 2, 513, 1, 5, "vqgan"))

VQ_N = (1, 31, 32, 33, 127, 128, 129, 257, 600, 657)


def vq_args():
    """(C, B, N, skip, nseg, with_stats): nseg from ds_vq_attn_segments for every N, and by hand: 4 at N = 657 (one block, six groups), 8 and 16
    at N = 600 (five groups: blocks of 3 + 2 with a ragged last tile; of 2 + 2 + 1 and an empty fourth), 4 * ngroups."""
    out = []
    for ci, C in enumerate((80, 160)):
        for i, N in enumerate(VQ_N):
            B = (1, 3)[(i + ci) % 2]
            skip = (i + ci) % 3 != 0
            out.append((C, B, N, skip, vq_segments_rule(B, N, C), i % 4 != 3))
        for N, ns, st in ((657, 4, True), (600, 8, True), (600, 16, True), (600, 20, False), (657, 24, True), (33, 8, True)):
            out.append((C, 3 if ns != 20 else 1, N, ns != 16 or C == 80, ns, st))
    return out


VQ_RANDOM = ((80, 3, 657, True), (160, 2, 257, False), (80, 1, 33, True), (160, 3, 600, True))
