"""Plain CPU helpers of tests/test_hip_codec_kernels.py and tests/test_codec_ref_cpu.py: the codec tail of csrc/tail.hip and
csrc/stft_codec.hpp (ds_vq_nearest, ds_vq_stats, ds_decoder_tail, ds_istft_plus, ds_istft_plus_loop, ds_stft_plus).

As in tests/support_ref.py four kinds of thing live here: case builders (preconditions asserted BEFORE anything is launched), float64
references (oracle/vocoder_ref.py and tests/decode_window_ref.py where they hold one), float32 restatements of each kernel's own arithmetic
("twins": the yardstick of the measured rule, never fitted to a device result) and defect models.

ds_vq_nearest, exact data.  At the ABI the contract is: the FIRST index that minimises d_j = esq[j] - 2 z . cb[j], and q = z + (cb[idx] - z).
The matrix-core search forms d_j from three bf16 parts per operand (h + m + l) with the products hh, hm, mh, mm, hl, lh per dimension and
the three parts of esq against 1.0.  On integer data with |esq[j]| + 2 sum_d |z_d| |cb[j][d]| < 2^24 at every (pixel, code) pair every one
of the 27 K-slot products is an integer and every fp32 partial sum is exact in any order; where the three dropped products (ml, lm, ll)
are zero as well (the builders assert it by emulating the split and the slot layout: vq_dist_parts) the kernel's distances ARE the float64
ones, so the indices equal the float64 first minimum at every pixel and q matches bit for bit.  The scalar kernel's (zz + esq) - 2 dot is
exact on the data sets whose |z|^2 also fits (all but `zlow`).

ds_vq_nearest, float data: the near-tie bound VQ_C.  With u = 2^-24 and S_j = |esq[j]| + 2 sum_d |z_d| |cb[j][d]|, the kernel's distance
of code j differs from the float64 d_j by at most
    dropped cross terms   a bf16 part is 8 bits wide: |m| <= 2^-8 (1 + 2^-8) |x|, |l| <= 2^-16 |x|, so |m_e l_z| + |l_e m_z| + |l_e l_z|
                          <= (2 (1 + 2^-8) + 2^-8) u |2 e_d| |z_d|: under 3 u S_j (one u per dropped product);
    truncation            what h + m + l leaves of an operand is at most u |x| (zero for a normal fp32 number: 3 x 8 bits hold its 24), on
                          z, on -2 cb and on esq: (2 u + u^2) 2 sum |z||e| + u |esq| <= 2.01 u S_j;
    accumulation          27 slot products summed in fp32, each addition within u of its partial sum, the partial sums within
                          (1 + 2^-8)^2 S_j (the parts' magnitudes): 27 x 1.01 u S_j <= 27.3 u S_j;
together under 33 u S_j.  Two distances are compared when a code is chosen over the float64 minimum, so the float64 distance of the chosen
code exceeds the float64 minimum by at most VQ_C u max(S_chosen, S_min) with VQ_C = 66.

The unit-norm bound UNIT_NORM_BOUND of ds_stft_plus.  stft_plus_encode rounds three times on the way to (c1, c2): the sum of squares
s^ = s (1 + t), |t| <= 2 u + u^2 (two products and a sum; fewer with a fused multiply-add), the square root n = sqrt(s^) (1 + d4): within
2 u of |X|, and the two divisions c = x / n (1 + d): c1^2 + c2^2 = s (1 + 2 d) / (s (1 + 2 . 2 u)) lies within 6 u + O(u^2) of 1:
UNIT_NORM_BOUND = 6 u (1 + 2^-20).  It holds wherever nothing underflows, which the power-of-two prescale of the encode ensures.

Perplexities are compared as ONE vector over all cases of a test: a single number under the measured rule is a coin toss (the twin's expf
can round exactly right, its distance be zero and the rule turn into bit equality with a library expf that is within an ulp)."""
import functools
import types

import numpy as np
import torch

import decode_window_ref as DW
import exact_ref as E
from oracle import vocoder_ref as V
from support_ref import _distinct_rows, _seed

U = 2.0 ** -24
VQ_C = 66.0
UNIT_NORM_BOUND = 6 * U * (1 + 2.0 ** -20)
NFFT = 1024
f32 = np.float32


# ================================================================================================= ds_vq_nearest: the split and the slots
def bf(v):
    """One round-to-nearest-even to bf16 of a float64 tensor of fp32-exact values, as float64."""
    return v.double().float().bfloat16().double()


def split3(v):
    """split3 of csrc/tail.hip on fp32-exact float64 values: h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m); both differences are
    exact in fp32 (asserted)."""
    assert E.is_f32(v)
    h = bf(v)
    r = v.double() - h
    assert E.is_f32(r)
    m = bf(r)
    assert E.is_f32(r - m)
    return h, m, bf(r - m)


def vq_dist_parts(z, cb, esq, drop=()):
    """The kernel's distance matrix [pixels][codes] from its K-slot layout, in float64 (exact on the integer data sets): code side
    -2 x (eh, eh, em, em, eh, el), pixel side (zh, zm, zh, zm, zl, zh), the three parts of esq against 1.  drop: parts a defective kernel
    loses ("z3": the pixel side's third part, "e3": the code side's, "q3": the third part of esq)."""
    zh, zm, zl = split3(z)
    eh, em, el = split3(-2.0 * cb)
    a, b, c = split3(esq)
    if "z3" in drop:
        zl = torch.zeros_like(zl)
    if "e3" in drop:
        el = torch.zeros_like(el)
    if "q3" in drop:
        c = torch.zeros_like(c)
    return zh @ eh.T + zm @ eh.T + zh @ em.T + zm @ em.T + zl @ eh.T + zh @ el.T + (a + b + c)[None]


def vq_dist64(z, cb, esq):
    return esq.double()[None] - 2.0 * (z.double() @ cb.double().T)


def first_min(d):
    """(index of the first minimum of every row, whether the minimum is attained more than once)."""
    dmin = d.min(1, keepdim=True).values
    hit = d == dmin
    n = d.shape[1]
    ar = torch.arange(n).expand_as(d)
    return torch.where(hit, ar, n).min(1).values, hit.sum(1) > 1


def last_min(d):
    hit = d == d.min(1, keepdim=True).values
    return torch.where(hit, torch.arange(d.shape[1]).expand_as(d), -1).max(1).values


def vq_twin_f32(z, cb, esq):
    """The matrix-core distance in fp32, slot by slot in the slot order (every bf16 x bf16 product is exact in fp32; each of the 27
    additions rounds once): [pixels][codes] float32.  z, cb, esq: fp32 tensors."""
    zh, zm, zl = (t.float() for t in split3(z.double()))
    eh, em, el = (t.float() for t in split3(-2.0 * cb.double()))
    parts = split3(esq.double())
    acc = torch.zeros(z.shape[0], cb.shape[0], dtype=torch.float32)
    for e, p in ((eh, zh), (eh, zm), (em, zh), (em, zm), (eh, zl), (el, zh)):
        for d in range(4):
            acc = acc + p[:, d:d + 1] * e[:, d][None]
    for t in parts:
        acc = acc + t.float()[None]
    return acc


def vq_bound(z, cb, esq):
    """S_j = |esq[j]| + 2 sum |z||cb[j]| per (pixel, code), float64."""
    return esq.double().abs()[None] + 2.0 * (z.double().abs() @ cb.double().abs().T)


def vq_excess(z, cb, esq, idx):
    """(float64 excess of the chosen code's distance over the minimum, the allowance VQ_C u max(S_chosen, S_min), float64 argmin)."""
    d = vq_dist64(z, cb, esq)
    ref, _ = first_min(d)
    s = vq_bound(z, cb, esq)
    r = torch.arange(d.shape[0])
    return d[r, idx] - d[r, ref], VQ_C * U * torch.maximum(s[r, idx], s[r, ref]), ref


def vq_q(z, cb, idx):
    """q = z + (cb[idx] - z) in fp32, two roundings."""
    zf, e = z.float(), cb.float()[idx]
    return zf + (e - zf)


# ================================================================================================= ds_vq_nearest: exact data sets
VQ_POOL = 515                                   # the largest B * HW of VQ_BHW
VQ_NCODES = (1, 15, 16, 17, 48, 64, 65, 100, 1000, 8192)
VQ_NCODES_SCALAR = (8193, 8200)
VQ_BHW = ((1, 1), (1, 15), (1, 16), (1, 17), (1, 128), (1, 129), (1, 512), (1, 513), (3, 5), (2, 77), (5, 103))
VQ_SETS = ("ties", "mid", "zlow", "elow")
VQ_MUTANTS = ("last_index", "groups_no_index", "z_third", "cb_third", "esq_third", "padding_wins", "b_half_tile")
# the data set on which a dropped-part defect is asked to show
VQ_MUTANT_SET = {"z_third": "zlow", "cb_third": "elow", "esq_third": "elow"}


def _with_duplicates(g, base_fn, ncodes):
    """ncodes rows: the first ceil(ncodes / 2) drawn by base_fn (distinct, none all zero), the others exact copies of seeded earlier rows:
    from two tiles on the last code tile holds duplicates of earlier codes only."""
    half = (ncodes + 1) // 2
    base = base_fn(half)
    src = torch.randint(0, half, (ncodes - half,), generator=g)
    return torch.cat([base, base[src]])


def _nonzero_rows(t, fill):
    t[(t == 0).all(1)] = fill
    return t


@functools.lru_cache(maxsize=None)
def vq_data(kind, ncodes):
    """One exact data set: z_pool [VQ_POOL][4], cb [ncodes][4], esq [ncodes] (float64 integers), the float64 first-minimum index of every
    pool pixel and its tie flag.  Pixel 0 is the zero vector and no code is: every distance there is esq[j] > 0, so a padding code of
    distance 0 would win.  Preconditions asserted: the margin, the emulated distances equal to float64, the part shares, the tie share."""
    g = E.gen(_seed("vq", kind, ncodes))
    P = VQ_POOL
    if kind == "ties":
        z = E.ints(g, (P, 4), -3, 3)
        cb = _with_duplicates(g, lambda n: _nonzero_rows(E.ints(g, (n, 4), -7, 7), 7.0), ncodes)
        esq = (cb * cb).sum(1)
    elif kind == "mid":
        z = E.ints(g, (P, 4), -1023, 1023)
        cb = _with_duplicates(g, lambda n: _nonzero_rows(E.ints(g, (n, 4), -1023, 1023), 1023.0), ncodes)
        esq = (cb * cb).sum(1)
    elif kind == "zlow":
        # few distinct codes (signed multiples of unit vectors, esq = s^2) and z whose coordinates differ by +-1 around a 19-bit base: the
        # largest coordinate decides, and the base's low bits live in the third part
        sign = E.choice(g, (P, 1), [-1.0, 1.0])
        z = sign * E.ints(g, (P, 1), 1 << 18, (1 << 19) - 2) + E.ints(g, (P, 4), -1, 1)
        s = E.choice(g, (ncodes,), [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
        cb = torch.zeros(ncodes, 4, dtype=torch.float64)
        cb[torch.arange(ncodes), torch.randint(0, 4, (ncodes,), generator=g)] = s
        esq = (cb * cb).sum(1)
    elif kind == "elow":
        # codes within +-2 of 64 centres (cluster j % 64; clusters k and k + 32 share a centre), esq the caller's array: one large base
        # (2^20 + 8192 a + 3008: the middle part is spent on the 3008) plus 1 .. 31 units per cluster, equal inside a cluster — between the two clusters of a centre the low bits of esq decide, inside a
        # cluster the low bits of the codes
        z = E.ints(g, (P, 4), -3, 3)
        centre = E.choice(g, (32, 4), [-1.0, 1.0]) * E.ints(g, (32, 4), 1 << 18, (1 << 19) - 3)
        k = torch.arange(ncodes) % 64
        cb = centre[k % 32] + E.ints(g, (ncodes, 4), -2, 2)
        ebase = float((1 << 20) + 8192 * int(E.ints(g, (1,), 0, 100).item()) + 3008)
        esq = ebase + E.ints(g, (64,), 1, 31)[k]
    else:
        raise ValueError(kind)
    z[0] = 0.0
    # ---- preconditions
    assert E.is_f32(z) and E.is_f32(cb) and E.is_f32(esq) and bool((esq > 0).all()) and not bool((cb == 0).all(1).any())
    margin = vq_bound(z, cb, esq).max().item()
    E.check_exact(margin)
    d = vq_dist64(z, cb, esq)
    assert torch.equal(vq_dist_parts(z, cb, esq), d), "a dropped cross term (ml, lm, ll) is not zero on this data"
    share = lambda t, i: (split3(t)[i] != 0).double().mean().item()                                       # noqa: E731
    shares = dict(z2=share(z, 1), z3=share(z, 2), e2=share(-2 * cb, 1), e3=share(-2 * cb, 2), q2=share(esq, 1), q3=share(esq, 2))
    if kind == "mid":
        assert shares["z2"] >= 0.25 and shares["e2"] >= 0.25, shares
    if kind == "zlow":
        assert shares["z3"] >= 0.25, shares
    if kind == "elow":
        assert shares["e3"] >= 0.25 and shares["q3"] >= 0.25, shares
    idx, tied = first_min(d)
    if kind == "ties" and ncodes >= 2:
        assert tied.double().mean().item() >= 0.25, tied.double().mean().item()
    zz = (z * z).sum(1).max().item()
    return types.SimpleNamespace(kind=kind, ncodes=ncodes, z=z, cb=cb, esq=esq, idx=idx, tied=tied, margin=margin, shares=shares, d=d,
                                 scalar_exact=zz + margin < E.LIMIT)


def vq_layout(z_pool, B, HW):
    """The first B * HW pool pixels as the [B][4][HW] tensor the kernel reads (pixel i = sample i // HW, position i % HW)."""
    return z_pool[:B * HW].view(B, HW, 4).permute(0, 2, 1).contiguous()


def vq_unlayout(q):
    """[B][4][HW] -> [B * HW][4]."""
    return q.permute(0, 2, 1).reshape(-1, 4)


def vq_mutant(c, kind):
    """The index of every pool pixel a matrix-core search with one fault would report, or None where the fault cannot show.
    last_index       <= in place of <: the last minimum wins (the tile examined again counts too);
    groups_no_index  the four lane groups of a pixel combined by distance alone: of equal distances the lower group wins, not the lower index;
    z_third / cb_third / esq_third   the third bf16 part of the pixel side, of the code side, of esq left out;
    padding_wins     the codes that pad the last tile at distance 0 instead of 3e38;
    b_half_tile      the B half (pixels 64 .. 127 of a wave's 128) examined with the tile number of the A half: one tile late, + 16, except in
                     the last tile (examined once more after the loop with its own number)."""
    n, d = c.ncodes, c.d
    ntiles = (n + 15) // 16
    if n > 8192:
        return None
    if kind == "last_index":
        return last_min(d)
    if kind == "groups_no_index":
        grp = (torch.arange(n) % 16) // 4
        best = torch.full((d.shape[0], 4), float("inf"), dtype=torch.float64)
        bi = torch.zeros(d.shape[0], 4, dtype=torch.long)
        for k in range(4):
            if bool((grp == k).any()):
                cols = (grp == k).nonzero().flatten()
                i, _ = first_min(d[:, cols])
                bi[:, k] = cols[i]
                best[:, k] = d[torch.arange(d.shape[0]), cols[i]]
        w, _ = first_min(best)
        return bi[torch.arange(d.shape[0]), w]
    if kind in ("z_third", "cb_third", "esq_third"):
        return first_min(vq_dist_parts(c.z, c.cb, c.esq, drop={"z_third": "z3", "cb_third": "e3", "esq_third": "q3"}[kind]))[0]
    if kind == "padding_wins":
        if n % 16 == 0:
            return None
        return first_min(torch.cat([d, torch.zeros(d.shape[0], 16 * ntiles - n, dtype=torch.float64)], 1))[0]
    if kind == "b_half_tile":
        i = torch.arange(d.shape[0])
        late = (i % 128 >= 64) & (c.idx // 16 < ntiles - 1)
        return c.idx + 16 * late
    raise ValueError(kind)


# ---- tied minima placed by construction
VQ_PLACED_PAIRS = ((36, 37), (82, 89), (135, 161), (7, 8188))
# (36, 37): two codes of one lane (tile 2, lane group 1, r = 0 and 1);  (82, 89): lane groups 0 and 2 of tile 5;  (135, 161): tiles 8 and 10 of
# one prefetch group of four, the LATER code in the lower lane group (combining the groups by distance alone would take it);  (7, 8188): the first and the last tile


@functools.lru_cache(maxsize=None)
def vq_placed_ties():
    """8192 distinct codes of +-1023 except that cb[b] = cb[a] for the four pairs above; 512 pixels (one block: four waves of eight pixel
    tiles); in every pixel tile the pixels 1, 5, 9, 13 sit exactly on cb[a] of pair 0, 1, 2, 3: each kind of tie is decided in both halves of
    every wave.  Asserted: the minimum of such a pixel is attained at exactly {a, b}."""
    g = E.gen(_seed("vq_placed"))
    cb = _distinct_rows(g, E.ints(g, (8192, 4), -1023, 1023), 1023)
    for a, b in VQ_PLACED_PAIRS:
        cb[b] = cb[a]
    z = E.ints(g, (512, 4), -1023, 1023)
    placed = {}
    for tile in range(32):
        for k, (a, b) in enumerate(VQ_PLACED_PAIRS):
            z[tile * 16 + 1 + 4 * k] = cb[a]
            placed[tile * 16 + 1 + 4 * k] = (a, b)
    esq = (cb * cb).sum(1)
    E.check_exact(vq_bound(z, cb, esq).max().item())
    d = vq_dist64(z, cb, esq)
    assert torch.equal(vq_dist_parts(z, cb, esq), d)
    idx, tied = first_min(d)
    for p, (a, b) in placed.items():
        hit = (d[p] == d[p].min()).nonzero().flatten().tolist()
        assert hit == [a, b] and idx[p] == a, (p, hit)
    return types.SimpleNamespace(kind="placed", ncodes=8192, z=z, cb=cb, esq=esq, idx=idx, tied=tied, d=d, placed=placed)


# ---- float data
VQ_FLOAT = (("uniform", 1.3), ("uniform", 100.0), ("normal", 1.3), ("normal", 100.0))
VQ_FLOAT_BHW = (2, 150)


@functools.lru_cache(maxsize=None)
def vq_float_case(book, zscale):
    """The production codebook's distribution uniform(-1 / 8192, 1 / 8192) or N(0, 0.7^2), 8192 codes, z = N(0, 1) x zscale x the codebook's
    scale; esq = the fp32 row sums of cb^2 as the module computes them."""
    g = E.gen(_seed("vq_float", book, zscale))
    if book == "uniform":
        cb = ((torch.rand(8192, 4, generator=g, dtype=torch.float64) * 2 - 1) / 8192).float()
        scale = 1.0 / 8192
    else:
        cb = (torch.randn(8192, 4, generator=g, dtype=torch.float64) * 0.7).float()
        scale = 0.7
    B, HW = VQ_FLOAT_BHW
    z = (torch.randn(B * HW, 4, generator=g, dtype=torch.float64) * zscale * scale).float()
    return types.SimpleNamespace(book=book, zscale=zscale, z=z, cb=cb, esq=torch.sum(cb ** 2, dim=1), B=B, HW=HW)


# ================================================================================================= ds_vq_stats
VQS_GRID = 2048 * 256
# (D, B, HW, ncodes, usage): npix 1, 255, 257 and a second trip of the 2048-block grid with a ragged tail; ncodes 1, 512, 1024, 1025 (a second
# trip of the finish loop), 8192
VQS_CASES = ((4, 1, 1, 1, "skew"), (1, 3, 85, 512, "skew"), (3, 1, 257, 1024, "skew"), (8, 1, 257, 1025, "high"), (4, 5, 51, 8192, "skew"),
             (1, 3, 174775, 1025, "high"), (4, 3, 85, 512, "one"), (3, 1, 256, 1025, "uniform"), (4, 3, 85, 1025, "outside"))
VQS_MUTANTS = ("grid_one_trip", "finish_one_trip", "outside_clamped", "counts_kept")


@functools.lru_cache(maxsize=None)
def vqs_case(D, B, HW, ncodes, usage):
    """Integer z and q of +-15 ([B][D][HW]) and indices: skew (a cubed uniform: unused codes), high (the upper codes as well, so that codes
    from 1024 on are used), one (every pixel on code ncodes - 1), uniform (64 codes, four pixels each: perplexity 64), outside (skew with a
    few indices of -1 and ncodes)."""
    g = E.gen(_seed("vqs", D, B, HW, ncodes, usage))
    npix = B * HW
    z = E.ints(g, (B, D, HW), -15, 15)
    q = E.ints(g, (B, D, HW), -15, 15)
    r = torch.rand(npix, generator=g, dtype=torch.float64)
    if usage in ("skew", "outside"):
        idx = (r ** 3 * min(ncodes, 300)).long()
    elif usage == "high":
        idx = ncodes - 1 - (r ** 3 * min(ncodes, 300)).long()
    elif usage == "one":
        idx = torch.full((npix,), ncodes - 1, dtype=torch.long)
    elif usage == "uniform":
        assert npix == 256
        idx = (torch.arange(256) % 64) * 16 + 5
    else:
        raise ValueError(usage)
    if usage == "outside":
        idx[torch.tensor([0, 7, npix - 1])] = -1
        idx[torch.tensor([3, 100])] = ncodes
        idx[11] = ncodes + 5
    assert int(idx.max()) < ncodes + 6 and ((q - z) ** 2).sum().item() < 2 ** 53
    if usage == "high" and ncodes > 1024:
        assert int((idx >= 1024).sum()) > 0
    return types.SimpleNamespace(D=D, B=B, HW=HW, ncodes=ncodes, usage=usage, npix=npix, z=z, q=q, idx=idx)


def vqs_counts(c, mutant=None):
    idx = c.idx
    if mutant == "grid_one_trip":
        idx = idx[:VQS_GRID]
    if mutant == "outside_clamped":
        idx = idx.clamp(0, c.ncodes - 1)
    ok = (idx >= 0) & (idx < c.ncodes)
    cnt = torch.bincount(idx[ok], minlength=c.ncodes)
    if mutant == "finish_one_trip":
        cnt = cnt[:1024]
    return cnt


def vqs_expect(c, cc, ema, mutant=None, before=None):
    """(mse, loss) bit for bit as fp32 tensors and the perplexity as (fp32 twin, float64).  mse: the float64 mean rounded once; loss: cc * mse
    or mse + cc * mse, one fp32 rounding per operation; the twin of the perplexity is the finish kernel's arithmetic: p = fp32(count /
    npix), the terms p * logf(p + 1e-10f) in fp32, their sum in double, expf of its fp32 negative.  before: the case whose counts a
    defective kernel would not have cleared ("counts_kept")."""
    ssum = ((c.q - c.z) ** 2).flatten(1)
    if mutant == "grid_one_trip":
        ssum = ((c.q - c.z) ** 2).sum(1).flatten()[:VQS_GRID]
    mse = torch.tensor(ssum.sum().item() / float(c.npix * c.D), dtype=torch.float64).float()
    ccf = torch.tensor(cc, dtype=torch.float32)
    loss = ccf * mse if ema else mse + ccf * mse
    cnt = vqs_counts(c, mutant).double()
    if mutant == "counts_kept":
        cnt = cnt + vqs_counts(before).double()
    p64 = cnt / c.npix
    perp64 = torch.exp(-(p64 * torch.log(p64 + 1e-10)).sum())
    p32 = p64.float()
    h = (p32 * torch.log(p32 + torch.tensor(1e-10, dtype=torch.float32))).double().sum()
    perp32 = torch.exp((-h).float())
    return mse, loss, perp32, perp64


# ================================================================================================= ds_decoder_tail
TAIL_GRID = 8192 * 256
TAIL_BIG = (2, (TAIL_GRID + 2048) // 2)           # (B, HW): 2,048 pixels more than one pass of the capped grid
TAIL_LADDER = (0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-8, -1e-8, 1.0, -1.0, 19.99, -19.99, 20.0, float(np.nextafter(f32(20), f32(np.inf))),
               88.0, -88.0, 104.0, -104.0, 1e30, -1e30)
TAIL_BAND = 31                                    # fp32 neighbours on either side of a ladder value that share its band


def tail_ladder_f32():
    """(values, band) fp32: every ladder value with its TAIL_BAND fp32 neighbours on either side; band = the ladder value's number.  A band
    is one comparison under the measured rule: its outputs are of one magnitude, so the norm weighs every element."""
    vals, band = [], []
    for k, v in enumerate(TAIL_LADDER):
        bits = int(np.array(v, dtype=f32).view(np.int32))
        mag, neg = bits & 0x7FFFFFFF, bits < 0
        for s in range(-TAIL_BAND, TAIL_BAND + 1):
            m = mag + s
            if m < 0:
                m, flip = -m, True
            else:
                flip = False
            x = np.array(m, dtype=np.int32).view(f32)
            vals.append(-x if neg != flip else x)
            band.append(k)
    v = torch.from_numpy(np.array(vals, dtype=f32))
    assert bool(torch.isfinite(v).all())
    for x in TAIL_LADDER:
        assert bool((v == float(f32(x))).any())
    return v, torch.tensor(band)


def tail_values_bf16():
    """(values, band): every finite bf16 of magnitude up to 128 as fp32; band = sign and octave: |x| in [2^k, 2^(k+1)) for k = -8 .. 6, 128
    with octave 6, everything below 2^-8 (zeros and denormals too) in one band per sign."""
    v = E.all_bf16_values()
    v = v[v.abs() <= 128]
    octave = torch.floor(torch.log2(v.abs().double().clamp_min(2.0 ** -9))).clamp(-9, 6).long() + 9
    neg = (v.view(torch.int32) < 0).long()
    assert v.numel() > 34000
    return v, octave * 2 + neg


def tail_input(vals, B, Cs, dtype):
    """[B][HW][Cs]: value i in channels 0, 1, 2 of pixel i (the list padded to a multiple of B with its first value), NaN in channels 3 up."""
    n = vals.numel()
    hw = (n + B - 1) // B
    full = torch.cat([vals, vals[:1].expand(B * hw - n)])
    x = torch.full((B, hw, Cs), float("nan"), dtype=dtype)
    x[..., :3] = full.view(B, hw, 1).to(dtype)
    return x, hw


def tail_twin(x):
    """The kernel's formulas in torch fp32 on [..., >= 3]: v0 > 20 ? v0 : log1pf(expf(v0)), tanhf, tanhf -> [B][3][HW]."""
    v = x[..., :3].float()
    sp = torch.where(v[..., 0] > 20.0, v[..., 0], torch.log1p(torch.exp(v[..., 0])))
    return torch.stack([sp, torch.tanh(v[..., 1]), torch.tanh(v[..., 2])], 1)


def tail_ref64(x, threshold=True):
    v = x[..., :3].float().double()
    sp = torch.nn.functional.softplus(v[..., 0]) if threshold else torch.log1p(torch.exp(v[..., 0]))
    return torch.stack([sp, torch.tanh(v[..., 1]), torch.tanh(v[..., 2])], 1)


def tail_groups(ref_rows, band, anchor):
    """The comparison groups of one output function: the bands, except that every band whose float64 outputs round to fewer than 32
    distinct fp32 values (softplus around 0: ln 2 throughout; a saturated tanh: 1 throughout) joins the band `anchor` (the one that holds
    x = 1).  The rule measures the precision of an fp32 evaluation; on a band of ONE output value the twin's distance is the luck of a
    single rounding.  ref_rows [rows][n] float64; -> group number per value."""
    group = band.clone()
    for k in band.unique().tolist():
        m = band == k
        if torch.unique(ref_rows[:, m].float()).numel() < 32:
            group[m] = anchor
    return group


def tail_anchor(vals, band):
    return int(band[(vals == 1.0).nonzero()[0, 0]])


# ================================================================================================= ds_istft_plus
ISTFT_SHAPES = ((2, 256), (2, 1024), (4, 256), (5, 256), (8, 128), (9, 128), (3, 512), (12, 256), (13, 256))
ISTFT_LOOP_SHAPES = ((8, 128), (2, 512), (4, 256))
ISTFT_B = (1, 3)


@functools.lru_cache(maxsize=None)
def istft_input(B, T):
    """[B][3][512][T] fp32: c0 = |N(0, 1)| / 2, (c1, c2) = N(0, 1) pairs (not of unit length, as the decoder's tanh outputs)."""
    g = torch.Generator().manual_seed(_seed("istft", B, T))
    enc = torch.randn(B, 3, 512, T, generator=g)
    enc[:, 0] = enc[:, 0].abs() * 0.5
    return enc


def decode_twin(c0, c1, c2):
    """stft_plus_decode in numpy fp32: expm1f, the pair scaled by an exact power of two, 1 / sqrt with one Newton step."""
    c0, c1, c2 = (np.asarray(t, dtype=f32) for t in (c0, c1, c2))
    mag = np.expm1(c0)
    pm = np.maximum(np.abs(c1), np.abs(c2))
    z0 = ~(pm > 0) | ~(pm < f32(3.0e38))
    pe = np.where(z0, 0, np.frexp(np.where(z0, f32(1), pm))[1]).astype(np.int32)
    pa, pb = np.ldexp(c1, -pe).astype(f32), np.ldexp(c2, -pe).astype(f32)
    n2 = pa * pa + pb * pb
    ri = f32(1) / np.sqrt(np.where(z0, f32(1), n2))
    ri = ri * (f32(1.5) - f32(0.5) * n2 * ri * ri)
    return np.where(z0, mag, mag * (pa * ri)).astype(f32), np.where(z0, f32(0), mag * (pb * ri)).astype(f32)


def _tw256():
    m = np.arange(256)
    return np.cos(2 * np.pi * m / NFFT).astype(f32), np.sin(2 * np.pi * m / NFFT).astype(f32)


def _cmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def frames_twin(enc):
    """istft_frames_r4_kernel in numpy fp32: the Hermitian spectrum from the decode twin, five radix-4 Stockham passes between two buffers
    with a 256-entry fp32 twiddle table (w^2 and w^3 by multiplication), 1 / 1024 and the periodic Hann window from the same table.
    enc [B][3][512][T] -> frames [B][T][1024] fp32."""
    e = np.asarray(enc, dtype=f32)
    B, _, F, T = e.shape
    dr, di = decode_twin(e[:, 0], e[:, 1], e[:, 2])                       # [B][F][T], bin kk = row + 1
    xr, xi = np.zeros((B, T, NFFT), f32), np.zeros((B, T, NFFT), f32)
    kk = np.arange(1, F + 1)
    xr[:, :, kk], xi[:, :, kk] = dr.transpose(0, 2, 1), di.transpose(0, 2, 1)
    xr[:, :, NFFT - kk[:-1]], xi[:, :, NFFT - kk[:-1]] = dr.transpose(0, 2, 1)[:, :, :-1], -di.transpose(0, 2, 1)[:, :, :-1]
    twr, twi = _tw256()
    tid = np.arange(256)
    for p, sh in ((1, 8), (4, 6), (16, 4), (64, 2), (256, 0)):
        k = tid & (p - 1)
        j = ((tid - k) << 2) + k
        w1 = (twr[k << sh], twi[k << sh])
        w2 = _cmul(w1, w1)
        w3 = _cmul(w2, w1)
        u0 = (xr[..., tid], xi[..., tid])
        u1 = _cmul((xr[..., tid + 256], xi[..., tid + 256]), w1)
        u2 = _cmul((xr[..., tid + 512], xi[..., tid + 512]), w2)
        u3 = _cmul((xr[..., tid + 768], xi[..., tid + 768]), w3)
        a0 = (u0[0] + u2[0], u0[1] + u2[1])
        a1 = (u0[0] - u2[0], u0[1] - u2[1])
        a2 = (u1[0] + u3[0], u1[1] + u3[1])
        a3 = (-(u1[1] - u3[1]), u1[0] - u3[0])
        yr, yi = np.empty_like(xr), np.empty_like(xi)
        for q, (s, t) in enumerate(((a0, a2), (a1, a3), (a0, a2), (a1, a3))):
            sg = f32(1) if q < 2 else f32(-1)
            yr[..., j + q * p], yi[..., j + q * p] = s[0] + sg * t[0], s[1] + sg * t[1]
        xr, xi = yr, yi
    n = np.arange(NFFT)
    m, qd = n & 255, n >> 8
    cs = np.select([qd == 0, qd == 1, qd == 2], [twr[m], -twi[m], -twr[m]], twi[m]).astype(f32)
    w = f32(0.5) - f32(0.5) * cs
    return (xr * f32(1.0 / NFFT) * w).astype(f32)


def frames_ref64(enc):
    """float64 irfft of the decoded spectrum (oracle/vocoder_ref.py) times the periodic Hann window: [B][T][1024]."""
    out = []
    for e in np.asarray(enc, dtype=np.float64):
        D = V.depad_stft(V.decode_stft(e))
        out.append((np.fft.irfft(D, n=NFFT, axis=0) * V.hann_periodic(NFFT)[:, None]).T)
    return np.stack(out)


def _hann(n, dtype):
    if dtype == f32:
        return f32(0.5) - f32(0.5) * np.cos(2 * np.pi * n / NFFT).astype(f32)
    return 0.5 - 0.5 * np.cos(2 * np.pi * n / NFFT)


def ola(frames, hop, dtype, mutant=None):
    """istft_ola_kernel on given frames [B][T][1024] in `dtype` (fp32: the twin, one rounding per operation in the kernel's order; float64:
    the reference of the overlap-add alone).  Defect model: "hop256" (frame positions computed with a hop of 256 whatever
    the hop is)."""
    fr = np.asarray(frames, dtype=dtype)
    B, T, _ = fr.shape
    L = hop * (T - 1)
    s = np.arange(L)
    pos = s + NFFT // 2
    h = 256 if mutant == "hop256" else hop
    t_hi = np.minimum(pos // h, T - 1)
    t_lo = np.where(pos - NFFT < 0, 0, (pos - NFFT + h) // h)
    y, wss = np.zeros((B, L), dtype), np.zeros((B, L), dtype)
    for k in range(NFFT // h + 1):
        t = t_lo + k
        n = pos - t * h
        ok = (t <= t_hi) & (t >= 0) & (n >= 0) & (n < NFFT)
        tc, nc = np.clip(t, 0, T - 1), np.clip(n, 0, NFFT - 1)
        w = _hann(nc, dtype)
        y = np.where(ok, y + fr[:, tc, nc], y)
        wss = np.where(ok, wss + w * w, wss)
    tiny = dtype(1.17549435e-38)
    return np.where(wss > tiny, y / np.where(wss > tiny, wss, dtype(1)), y).astype(dtype)


def ola_loop(frames, hop, dtype):
    """istft_ola_loop_kernel on given frames: one period of hop * T samples, the addends in the order of the position inside the frame."""
    fr = np.asarray(frames, dtype=dtype)
    B, T, _ = fr.shape
    L = hop * T
    pos = np.arange(L) + NFFT // 2
    y, wss = np.zeros((B, L), dtype), np.zeros((B, L), dtype)
    for k in range(NFFT // hop):
        n = pos % hop + k * hop
        t = ((pos - n) // hop) % T
        w = _hann(n, dtype)
        y = y + fr[:, t, n]
        wss = wss + w * w
    return (y / wss).astype(dtype)


def istft_ref64(enc, hop):
    return np.stack([V.istft(V.depad_stft(V.decode_stft(e)), hop, NFFT) for e in np.asarray(enc, dtype=np.float64)])


def istft_loop_ref64(enc, hop):
    return np.stack([DW.istft_loop(V.depad_stft(DW.decode(e)), hop) for e in np.asarray(enc, dtype=np.float64)])


# ================================================================================================= ds_stft_plus
STFT_CASES = ((513, 256, ("reflect",)), (1000, 256, ("constant", "reflect")), (2560, 256, ("constant", "reflect")), (2048, 128, ("constant",)),
              (2048, 512, ("reflect",)), (1500, 100, ("constant",)), (1, 256, ("constant",)))
STFT_TOUT_B = ((0, 3), (1, 1), (7, 3))             # (T_out - T, B)
STFT_MUTANTS = ("reflect_as_constant", "tail_wraps", "encode_unscaled")


@functools.lru_cache(maxsize=None)
def stft_audio(B, L):
    return torch.randn(B, L, generator=torch.Generator().manual_seed(_seed("stft", B, L)))


def stft_frames_of(audio, hop, reflect, dtype, mutant=None):
    """The gathered, windowed frames [B][T][1024] of the kernel: centred, zero or reflect padding."""
    y = np.asarray(audio, dtype=dtype)
    B, L = y.shape
    T = 1 + L // hop
    i = np.arange(T)[:, None] * hop + np.arange(NFFT)[None] - NFFT // 2
    if mutant == "tail_wraps":
        i = np.where(i >= L, i - L, i)
    if reflect and mutant != "reflect_as_constant":
        i = np.where(i < 0, -i, i)
        i = np.where(i >= L, 2 * (L - 1) - i, i)
    ok = (i >= 0) & (i < L)
    v = np.where(ok[None], y[:, np.clip(i, 0, L - 1)], dtype(0))
    return (v * _hann(np.arange(NFFT), dtype)).astype(dtype)


def stft_ref64(audio, hop, reflect):
    """The float64 transform of the same fp32 audio, bins 1 .. 512: complex128 [B][512][T].  (Equal to oracle/vocoder_ref.stft before its
    rounding to complex64: test_codec_ref_cpu.py holds the two together.)"""
    fr = stft_frames_of(audio, hop, reflect, np.float64)
    return np.fft.rfft(fr, axis=-1)[..., 1:].transpose(0, 2, 1)


def encode_twin(xr, xi, prescale=True):
    """stft_plus_encode in numpy fp32.  prescale: the pair scaled by an exact power of two so that max(|xr|, |xi|) lies in [0.5, 1) before
    it is squared (the kernel's form); without it the squares of a quiet bin are denormal or zero: the defect model "encode_unscaled"."""
    xr, xi = np.asarray(xr, dtype=f32), np.asarray(xi, dtype=f32)
    pm = np.maximum(np.abs(xr), np.abs(xi))
    z0 = ~(pm > 0)
    pe = np.where(z0, 0, np.frexp(np.where(z0, f32(1), pm))[1]).astype(np.int32) if prescale else np.zeros(pm.shape, np.int32)
    pa, pb = np.ldexp(xr, -pe).astype(f32), np.ldexp(xi, -pe).astype(f32)
    n = np.sqrt(pa * pa + pb * pb)
    mag = np.ldexp(n, pe).astype(f32)
    live = n > 0
    safe = np.where(live, n, f32(1))
    return np.log1p(mag), np.where(live, pa / safe, f32(1)).astype(f32), np.where(live, pb / safe, f32(0)).astype(f32)


def stft_twin(audio, hop, reflect, T_out=None, mutant=None):
    """stft_plus_kernel in numpy fp32: radix-2 decimation in time on the bit-reversed windowed frame, fp32 twiddles per butterfly, then the
    encode twin; columns past the signal's frames are (0, 1, 0).  -> [B][3][512][T_out] fp32."""
    fr = stft_frames_of(audio, hop, reflect, f32, mutant)
    B, T, _ = fr.shape
    rev = np.array([int(format(n, "010b")[::-1], 2) for n in range(NFFT)])
    re, im = np.zeros_like(fr), np.zeros_like(fr)
    re[..., rev] = fr
    ln = 2
    while ln <= NFFT:
        half = ln >> 1
        j = np.arange(NFFT // 2)
        grp, pos = j // half, j % half
        i0 = grp * ln + pos
        i1 = i0 + half
        ang = -2.0 * np.pi * pos / ln
        c, s = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
        tr = re[..., i1] * c - im[..., i1] * s
        ti = re[..., i1] * s + im[..., i1] * c
        ur, ui = re[..., i0].copy(), im[..., i0].copy()
        re[..., i0], im[..., i0] = ur + tr, ui + ti
        re[..., i1], im[..., i1] = ur - tr, ui - ti
        ln <<= 1
    c0, c1, c2 = encode_twin(re[..., 1:513], im[..., 1:513], prescale=mutant != "encode_unscaled")
    T_out = T if T_out is None else T_out
    out = np.zeros((B, 3, 512, T_out), f32)
    out[:, 1] = 1
    for ch, v in enumerate((c0, c1, c2)):
        out[:, ch, :, :T] = v.transpose(0, 2, 1)
    return out


def spectrum_of(enc):
    """expm1(c0) * (c1, c2) of an fp32 representation in float64: complex128 [B][512][T]."""
    e = np.asarray(enc, dtype=np.float64)
    return np.expm1(e[:, 0]) * (e[:, 1] + 1j * e[:, 2])


def per_frame(z, ref):
    """z and ref (complex [B][512][T]) divided by the largest |ref| of each frame (1 where the frame is silent), as real tensors
    [B][512][T][2]: under conftest.rel_err every bin then counts against the strongest bin of ITS frame, the weak ones included."""
    top = np.abs(ref).max(axis=1, keepdims=True)
    top = np.where(top > 0, top, 1.0)
    pack = lambda a: torch.from_numpy(np.stack([(a / top).real, (a / top).imag], -1))                     # noqa: E731
    return pack(z), pack(ref)
