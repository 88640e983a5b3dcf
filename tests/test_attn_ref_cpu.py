"""No GPU: what tests/test_hip_attn_paths.py relies on.  Every case it launches meets the preconditions of exactness (asserted by the builder
of tests/attn_ref.py, re-checked and measured here), the step-by-step fp32 restatement of every kernel form equals the float64 reference
bit for bit, every defect model changes the expectation of a NAMED case, the path predicates agree with a thread-by-thread restatement of
the kernels' tile ranges, and every kernel form meets every predicate asked of it in at least one case."""
import torch

import attn_ref as R
import exact_ref as E

CASES = R.gpu_cases()


def _all():
    for k in CASES:
        yield k, R.build(k), R.forms(k), R.resolve_nseg(k)


def test_every_case_meets_its_preconditions():
    ids = [R.case_id(k) for k in CASES]
    assert len(set(ids)) == len(ids)
    wide = small = 0
    for k, c, (cf, of, batch), nseg in _all():
        assert c.B == k["B"] and c.N == k["N"] and c.C == k["C"]
        # operands and every packed intermediate: exact in bf16 (the builder asserts it; the margin of every sum against 2^24)
        E.check_exact(max(c.margin_proj, c.margin_ctx, c.margin_z))
        assert E.is_bf16(c.want_ctx.double()) and E.is_f32(c.z64)
        # every column has a selected pixel, counts are powers of two, and the label decides rows where there is one
        assert bool(c.ksel.any(1).all())
        if c.label_full is not None:
            assert bool(torch.isnan(c.label_full[:, 128:]).all()) and c.lq_stride > 128
            if c.B > 1:
                assert not torch.equal(c.label_full[0, :128], c.label_full[1, :128]), "samples must differ in their label"
        # tiles whose own maximum is an unselected key: wanted wherever there is more than one tile
        if c.N > 64:
            tiles = c.ksel[:, :c.N // 32 * 32].view(c.B, -1, 32, 128).any(2)
            assert not bool(tiles.all()), "some (tile, column) must hold no selected pixel"
        if c.wide:
            E.check_rounding(c.z64)
            wide += 1
        else:
            assert c.stats_exact, (R.case_id(k), c.stats_margin)
            small += 1
        # exact GroupNorm partials: the kernels' own float64 reduction returns (a, a mean) exactly
        part, count, eps = R.gn_partials(c)
        s = part.double().sum(1)
        mean = s[:, 0] / count
        a = 1.0 / torch.sqrt(s[:, 1] / count - mean * mean + eps)
        assert torch.equal(a, c.a) and torch.equal(a * mean, c.a * c.mean)
        # no block of the output pass without a tile: no idle statistics slot exists in this tier
        assert all(any(len(w) for w in blk) for blk in R.out_block_tiles(of, c.N, c.C, batch))
    assert wide >= 20 and small >= 20


def test_restatements_equal_the_reference():
    """The fp32 walk of every context form (segments, tiles, lane halves, rescale, partials, combine) and of every output form (q softmax,
    bf16 packs, Y resp. M_b) on every case, against float64 rounded once."""
    seen = set()
    for k, c, (cf, of, batch), nseg in _all():
        assert torch.equal(R.ctx_walk(c, cf, nseg), c.want_ctx), R.case_id(k)
        assert torch.equal(R.out_walk(c, of), c.want_y), R.case_id(k)
        # both generations meet the one reference on every case they exist for
        for of2 in (("out", c.C // 16, R.group_t(c.C, c.N)), ("out2", c.C // 16)):
            assert torch.equal(R.out_walk(c, of2), c.want_y)
        tot = R.block_stats(c, of, batch, rounded=(of[0] == "out2")).sum(1)
        assert torch.equal(tot, c.stats_y if of[0] == "out2" else c.stats_z)
        seen.add(cf)
        seen.add(of)
    assert seen == set(FORMS), sorted(seen ^ set(FORMS))


# defect -> (case that must change, what is compared)
NAMED = {
    "ragged_unmasked": "C96_B1_N33_gen1_s2_h0_wide_ab",
    "drop_last_tile": "C192_B2_N33_gen2_s2_h0_wide_ab",
    "stale_empty_segment": "C96_B1_N127_gen1_s8_h0_wide_ab",
    "rescale_skipped": "C96_B2_N129_gen1_s3_h0_wide_ab",
    "halves_max_not_shared": "C384_B1_N129_gen1_s3_h0_wide_ab",
    "t2_first_tile_bound": "C96_B1_N4129_gen1_slib_h0_small_ab",
    "wout_heads_swapped": "C96_B2_N31_gen1_s2_h0_wide_ab",
    "lq_stride_ignored": "C96_B2_N31_gen1_s2_h0_wide_ab",
    "scale_dropped": "C192_B1_N129_gen2_s8_h0_wide_ab",
    "bias_dropped": "C96_B3_N32_gen1_s1_h0_small_ab",
    "gn_part_wrong_count": "C96_B1_N129_gen1_s2_h0_wide_nomfold_part",
}


def test_every_defect_changes_a_named_case():
    assert set(NAMED) == set(R.CTX_DEFECTS + R.OUT_DEFECTS + R.GN_DEFECTS)
    by_id = {R.case_id(k): k for k in CASES}
    for d, cid in NAMED.items():
        k = by_id[cid]
        c, (cf, of, batch), nseg = R.build(k), R.forms(k), R.resolve_nseg(k)
        if d in R.CTX_DEFECTS:
            got = R.ctx_walk(c, cf, nseg, defect=d)
            assert not torch.equal(got, c.want_ctx), d
            if bool(torch.isfinite(got).all()):              # ... and it reaches y through the output pass
                assert not torch.equal(R.out_walk(c, of, got), c.want_y), d
        elif d in R.OUT_DEFECTS:
            assert not torch.equal(R.defect_y(c, d), c.want_y), d
        else:
            assert k["gn"] == "part" and not torch.equal(R.gn_wrong_count(c), c.want_ctx), d
    # each ctx defect is also seen in BOTH generations somewhere (the parts are shared, the masks and ranges are not)
    for d in ("ragged_unmasked", "drop_last_tile", "stale_empty_segment", "rescale_skipped", "halves_max_not_shared"):
        hit = set()
        for k, c, (cf, of, batch), nseg in _all():
            if cf[0] not in hit and not torch.equal(R.ctx_walk(c, cf, nseg, defect=d), c.want_ctx):
                hit.add(cf[0])
        assert hit == {"ctx", "ctx2"}, (d, hit)
    assert len(R.NOT_MODELLED) == 4


def _threads_ctx(form, N, nseg):
    """attn_fused_ctx_kernel / attn_ctx2_kernel block by block, wave by wave: (tiles per segment, waves that return without a partial)."""
    if form[0] == "ctx":
        T = form[2]
        TP = 32 * T
        ngroups = (N + TP - 1) // TP
        per = (ngroups + nseg - 1) // nseg
        segs = []
        for seg in range(nseg):                              # grid.x = nseg, the four waves of a block are the heads of ONE segment
            g0 = seg * per
            g1 = min(ngroups, g0 + per)
            tiles = []
            g = g0
            while g < g1:
                tiles += [(g * TP + t * 32) // 32 for t in range(T)]
                g += 1
            segs.append(tiles)
        return segs, 0
    C = form[1] * 16
    NW, HPW, HG = {96: (4, 4, 1), 192: (8, 4, 1), 384: (8, 2, 2)}[C]
    HB = 4 // HG
    NSB = NW * HPW // HB
    ntiles = (N + 31) >> 5
    per = (ntiles + nseg - 1) // nseg
    segs, past = {}, 0
    for bx in range((nseg + NW - 1) // NW):
        for z in range(HG):
            for wave in range(NW):
                seg = bx * NSB + wave % NSB
                t0 = min(ntiles, seg * per)
                t1 = min(ntiles, t0 + per)
                t1f = t1 - 1 if (t1 == ntiles and (N & 31)) else t1
                tiles = list(range(t0, t1f)) + ([t1f] if (t1f < t1 and t1f >= t0) else [])
                if seg >= nseg:
                    past += 1
                    continue
                heads = tuple(range(z * HB + (wave // NSB) * HPW, z * HB + (wave // NSB) * HPW + HPW))
                segs.setdefault(seg, {})
                for h in heads:
                    assert h not in segs[seg]
                    segs[seg][h] = tiles
    out = []
    for seg in range(nseg):
        assert sorted(segs[seg]) == [0, 1, 2, 3], "every head of every segment has exactly one wave"
        assert all(segs[seg][h] == segs[seg][0] for h in range(4))
        out.append(segs[seg][0])
    return out, past


def _threads_out(form, N, C, batch):
    if form[0] == "out":
        T = form[2]
        TP = 32 * T
        ngroups = (N + TP - 1) // TP
        nb = R.out_blocks(ngroups, batch, C)
        per = (ngroups + nb - 1) // nb
        return [[[g * T + t for g in range(bx * per, min(ngroups, bx * per + per)) for t in range(T)]] for bx in range(nb)]
    NW = {96: 4, 192: 8}[C]
    nb = R.attn_out2_blocks(N, batch, C)
    ntiles = (N + 31) // 32
    per = (ntiles + nb - 1) // nb
    blocks = []
    for bx in range(nb):
        t0 = bx * per
        t1 = min(ntiles, t0 + per)
        waves = []
        for wave in range(NW):
            tiles, t = [], t0 + wave
            while t < t1:
                tiles.append(t)
                t += NW
            waves.append(tiles)
        blocks.append(waves)
    return blocks


def test_predicates_agree_with_the_thread_restatement():
    for C in (96, 192, 384):
        for N in (1, 31, 32, 33, 64, 65, 127, 129, 257, 1056, 1057, 4101, 4129):
            for nseg in (1, 2, 3, 8, 33, 65):
                for gen in (1, 2):
                    cf = R.ctx_form(1, N, C, gen)
                    segs, past = _threads_ctx(cf, N, nseg)
                    assert segs == R.ctx_segment_tiles(cf, N, nseg), (cf, N, nseg)
                    # every real pixel is walked exactly once
                    flat = [t for s in segs for t in s if t * 32 < N]
                    assert flat == list(range((N + 31) // 32)), (cf, N, nseg)
                    paths = R.ctx_paths(cf, N, nseg)
                    assert ("wave_past_nseg" in paths) == (past > 0)
                    assert ("empty_segment" in paths) == any(not s for s in segs)
            for batch in (1, 2, 3, 32, 96, 256, 512):
                for gen in (1, 2):
                    of = R.out_form(1, N, C, gen)
                    blocks = _threads_out(of, N, C, batch)
                    assert blocks == R.out_block_tiles(of, N, C, batch)
                    flat = sorted(t for b in blocks for w in b for t in w if t * 32 < N)
                    assert flat == list(range((N + 31) // 32)), (of, N, batch)
                    assert len(blocks) == R.stats_parts(1, N, C, gen, batch)
                    paths = R.out_paths(of, N, C, batch)
                    assert ("wave_without_tile" in paths) == any(not w for b in blocks for w in b)


FORMS = {
    ("ctx", 6, 1): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "all_but_one_empty", "several_segments"},
    ("ctx", 6, 2): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "t2_ragged_second_tile", "t2_second_tile_past_n"},
    ("ctx", 12, 1): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile"},
    ("ctx", 24, 1): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile"},
    ("ctx2", 6): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "wave_past_nseg", "several_segments"},
    ("ctx2", 12): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "wave_past_nseg", "several_segments"},
    ("ctx2", 24): {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "wave_past_nseg"},
    ("out", 6, 1): {"one_group_block", "several_trips", "one_block_all_groups", "ragged_last_tile", "several_blocks", "odd_groups", "even_groups"},
    ("out", 6, 2): {"one_group_block", "several_trips", "one_block_all_groups", "ragged_last_tile", "several_blocks", "odd_groups", "t2_ragged_second_tile", "t2_second_tile_past_n"},
    ("out", 12, 1): {"one_group_block", "several_trips", "one_block_all_groups", "ragged_last_tile", "several_blocks", "odd_groups", "even_groups"},
    ("out", 24, 1): {"one_group_block", "several_trips", "one_block_all_groups", "ragged_last_tile", "several_blocks", "odd_groups", "even_groups"},
    ("out2", 6): {"wave_without_tile", "several_trips", "ragged_last_tile", "several_blocks"},
    ("out2", 12): {"wave_without_tile", "several_trips", "ragged_last_tile", "several_blocks"},
}


def test_every_form_meets_every_predicate():
    have = {f: set() for f in FORMS}
    stats = {f: 0 for f in FORMS if f[0].startswith("out")}
    gn_part, gen0 = set(), set()
    for k, c, (cf, of, batch), nseg in _all():
        have[cf] |= R.ctx_paths(cf, c.N, nseg)
        have[of] |= R.out_paths(of, c.N, c.C, batch)
        stats[of] += c.stats_exact
        if k["gn"] == "part":
            gn_part |= {cf, of}
        if k["gen"] == 0:
            gen0.add((k["C"], R.generations(k["B"], k["N"], k["C"], 0, k["hint"], k["mfold"])))
    for f, need in FORMS.items():
        assert need <= have[f], (f, sorted(need - have[f]))
    assert all(n >= 1 for n in stats.values()), stats                  # exact statistics slots for every output form
    assert {f[0] for f in gn_part} == {"ctx", "ctx2", "out", "out2"}
    # gen = 0 picks each generation on each side of each threshold
    assert gen0 >= {(96, 0), (96, 2), (96, 3), (192, 0), (192, 3), (96, 1), (384, 1), (384, 0)}, gen0
    at1056 = {k["hint"] for k in CASES if k["gen"] == 0 and k["C"] == 384 and k["N"] >= 1024}
    assert at1056 >= {95, 96}, "C = 384 where the second-generation context exists: both sides of its threshold"


def test_launch_rules_hold_the_header_limits():
    """nseg may exceed the tile count (the surplus segments are empty and carry weight 0), and the second-generation count never does."""
    for C in (96, 192, 384):
        for B in (1, 2, 96, 600):
            for N in (1, 33, 1056, 4129):
                for gen in (0, 1, 2):
                    s = R.segments_gen(B, N, C, gen)
                    assert 1 <= s <= 64
                    if R.use_ctx2(B, N, C, gen):
                        assert s <= (N + 31) // 32


# ================================================================================================= the split-precision tier
X3 = R.x3_gpu_cases()

X3_NAMED = {
    "x_lo_w_hi_dropped": "x3_C96_B2_N33_s2_h0_wlo_ab",
    "v_lo_dropped": "x3_C192_B1_N129_s8_h0_wlo_part",
    "mb_lo_dropped": "x3_C384_B2_N33_s2_h0_wlo_ab",
    "q_lo_dropped": "x3_C96_B3_N65_s3_h0_qlo_ab",
    "lq_stride_ignored": "x3_C96_B2_N257_slib_h0_small_ab",
    "form_b_stats_of_pass2": "x3_C192_B2_N257_slib_h0_small_ab",
    "out_planes_lo_truncated": "x3_C96_B2_N33_s2_h0_wlo_ab",
}


def test_x3_cases_meet_their_preconditions_and_the_walk_equals_the_reference():
    ids = [R.x3_case_id(k) for k in X3]
    assert len(set(ids)) == len(ids)
    flav = set()
    for k in X3:
        c = R.x3_build(k)                                    # (the builder asserts keys, queries, margins and the shares of its flavour)
        nseg = R.x3_resolve_nseg(k)
        flav.add((c.C, c.flavour))
        assert max(c.margin_proj, c.margin_ctx, c.margin_z) < E.LIMIT
        assert torch.equal(R.x3_ctx_walk(c, nseg), c.want_ctx), R.x3_case_id(k)
        y, planes = R.x3_out_walk(c)                         # the fold and pass 2, fp32 step by step
        assert torch.equal(y, c.want_y) and torch.equal(planes, c.want_mfold), R.x3_case_id(k)
        if c.flavour == "wlo":
            assert c.share["x_lo"] >= 0.5 and c.share["x_wide3"] >= 0.05 and c.share["wv_lo"] >= 0.9 and c.share["v_lo"] >= 0.5 and c.share["mb_lo"] >= 0.5
        if c.flavour == "small":
            assert c.stats_exact
            tot = R.x3_block_stats(c, R.fused_batch(k["B"], k["hint"])).sum(1)
            assert torch.equal(tot, c.stats_z)
    assert flav == {(C, f) for C in (96, 192, 384) for f in ("wlo", "qlo", "small")}


def test_x3_every_defect_changes_a_named_case():
    assert set(X3_NAMED) == set(R.X3_DEFECTS)
    by_id = {R.x3_case_id(k): k for k in X3}
    for d, cid in X3_NAMED.items():
        k = by_id[cid]
        c = R.x3_build(k)
        batch = R.fused_batch(k["B"], k["hint"])
        g = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.arange(c.C) % 3]
        be = (torch.arange(c.C) % 5 - 2).double()
        if d == "form_b_stats_of_pass2":
            slots = R.x3_block_stats(c, batch)
            out, _, _ = R.x3_form_b(c, slots, g, be, 1e-5)
            bad, _, _ = R.x3_form_b(c, R.x3_block_stats(c, batch, out.double()), g, be, 1e-5)     # the statistics of what pass 2 forms
            assert not torch.equal(out, bad)
        elif d == "out_planes_lo_truncated":
            slots = R.x3_block_stats(c, batch)
            _, _, lo = R.x3_form_b(c, slots, g, be, 1e-5)
            _, _, lo_t = R.x3_form_b(c, slots, g, be, 1e-5, split=E.trunc_split)
            assert not torch.equal(lo, lo_t)
        else:
            assert not torch.equal(R.x3_defect_y(c, d), c.want_y), d
            if d in ("mb_lo_dropped", "q_lo_dropped"):      # ... and at its step of the fp32 restatement, with the same result
                assert torch.equal(R.x3_out_walk(c, defect=d)[0], R.x3_defect_y(c, d)), d
    # the walk's own faults, seen by the context of a named case
    k = by_id["x3_C192_B2_N33_s2_h0_wlo_ab"]
    c = R.x3_build(k)
    for d in ("ragged_unmasked", "drop_last_tile"):
        assert not torch.equal(R.x3_ctx_walk(c, 2, defect=d), c.want_ctx), d
    k = by_id["x3_C96_B1_N1057_slib_h512_wlo_ab"]             # segments of five tiles: the maximum moves inside a segment
    assert not torch.equal(R.x3_ctx_walk(R.x3_build(k), R.x3_resolve_nseg(k), defect="rescale_skipped"), R.x3_build(k).want_ctx)


def test_x3_predicates_and_coverage():
    # the tile ranges, wave by wave (attn_x3_pass1: seg = block * 8 + wave; attn_x3_z / _qz: t0 + wave, step 8)
    for N in (1, 33, 65, 129, 257, 1056, 1057):
        ntiles = (N + 31) // 32
        for nseg in (1, 2, 3, 8, 9, 65):
            per = (ntiles + nseg - 1) // nseg
            segs, past = [], 0
            for sb in range((nseg + 7) // 8):
                for wave in range(8):
                    seg = sb * 8 + wave
                    t0 = min(ntiles, seg * per)
                    t1 = min(ntiles, t0 + per)
                    if seg >= nseg:
                        assert t0 == t1
                        past += 1
                    else:
                        segs.append(list(range(t0, t1)))
            assert segs == R.x3_pass1_tiles(N, nseg) and [t for s in segs for t in s] == list(range(ntiles))
            assert ("wave_past_nseg" in R.x3_ctx_paths(96, N, nseg)) == (past > 0)
        for C in (192, 384):
            for B in (1, 3, 600):
                nq = R.x3_q_only_segments(B, N, C)
                assert [t for s in R.x3_pass1_tiles(N, nq) for t in s] == list(range(ntiles)), "the q-only launch projects every tile once"
        for C in (96, 192, 384):
            for batch in (1, 2, 3, 256, 512):
                per = R.z_tiles_per_block(N, batch, C)
                nb = (ntiles + per - 1) // per
                blocks = [[[t for t in range(tb * per + w, min(ntiles, tb * per + per), 8)] for w in range(8)] for tb in range(nb)]
                assert blocks == R.x3_out_block_tiles(N, C, batch)
                assert sorted(t for b in blocks for w in b for t in w) == list(range(ntiles))
                assert all(any(w for w in b) for b in blocks), "no block without a tile: every statistics slot has a writer with work"
                assert nb * (C // 96) == R.x3_stats_parts(1, N, C, batch)
    need_ctx = {"empty_segment", "one_group_segment", "odd_groups", "even_groups", "ragged_last_tile", "wave_past_nseg", "several_segments"}
    need_out = {"wave_without_tile", "several_trips", "ragged_last_tile", "several_blocks"}
    for C in (96, 192, 384):
        have_c, have_o = set(), set()
        for k in X3:
            if k["C"] == C:
                have_c |= R.x3_ctx_paths(C, k["N"], R.x3_resolve_nseg(k), k["B"])
                have_o |= R.x3_out_paths(k["N"], C, R.fused_batch(k["B"], k["hint"]))
        assert need_ctx <= have_c, (C, sorted(need_ctx - have_c))
        assert need_out <= have_o, (C, sorted(need_out - have_o))
        if C != 96:
            assert "q_only_wave_without_tile" in have_c
