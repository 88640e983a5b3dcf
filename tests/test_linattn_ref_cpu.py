"""tests/linattn_ref.py checked without a GPU: every case of tests/test_hip_linattn_paths.py meets its preconditions, every exact reference is
reproduced bit for bit by fp32 evaluations in other summation orders (the proof that the data is exact), every defect model changes the
tensor a named GPU case compares, and the path predicates the shapes were chosen by agree with a thread-by-thread restatement of the launch
arithmetic of csrc/linattn.hip and csrc/vq_attn.hip."""
import pytest
import torch

import exact_ref as E
import linattn_ref as R

LIN_ARGS = R.linattn_args()
VQ_ARGS = R.vq_args()


LIN_BY_ID = {R.linattn_case(**a).id: a for a in LIN_ARGS}


def _lin(case_id):
    assert case_id in LIN_BY_ID, "not a case of the GPU test: %s" % case_id
    return R.linattn_case(**LIN_BY_ID[case_id])


def test_the_exponentials_the_argument_rests_on_are_exact_in_fp32():
    t = lambda v: torch.tensor(v, dtype=torch.float32)                                                    # noqa: E731
    assert torch.exp(t(0.0)).item() == 1.0 and torch.exp(t(-200.0)).item() == 0.0 and torch.exp(t(-400.0)).item() == 0.0
    assert torch.exp2(t(-288.5)).item() == 0.0 and torch.exp2(t(-200.0) * t(1.44269504088896340736)).item() == 0.0
    assert (1.0 / t(16.0)).item() * 16 == 1.0 and (t(0.25) * (1.0 / t(32.0))).double().item() == 2.0 ** -7


# ================================================================================================= linattn
def test_linattn_case_ids_are_distinct():
    ids = [R.linattn_case(**a).id for a in LIN_ARGS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("a", LIN_ARGS, ids=lambda a: R.linattn_case(**a).id)
def test_linattn_case_is_exact_in_any_order(a):
    c = R.linattn_case(**a)                                                      # (the builder asserted the preconditions)
    R.linattn_preconditions(c)
    ctx64, out64 = R.linattn_ref64(c)
    assert torch.equal(ctx64, c.want_ctx), "the float64 softmax formula, rounded once, is the hard selection"
    out_once = out64.float()                                                     # (weights of 1e-87 leave 1e-85 where the exact value is 0)
    assert torch.equal(out_once.bfloat16() if c.bf16 else out_once, c.want_out)
    for nseg in sorted({c.nseg, 1, min(c.N, 5)}):                                # the kernel's segments, one segment, five
        ctx32 = R.linattn_ctx_walk(c, nseg=nseg)
        assert ctx32.dtype == torch.float32 and torch.equal(ctx32, c.want_ctx), nseg
    out32 = R.linattn_out_walk(c, c.want_ctx)
    assert out32.dtype == torch.float32 and torch.equal(out32.double(), c.out)
    k, v = c.k.float().permute(0, 2, 3, 1), c.v.float().permute(0, 2, 3, 1)      # torch's own fp32 softmax, the token appended FIRST
    if c.token:
        k, v = torch.cat([c.lk.float().unsqueeze(-1), k], -1), torch.cat([c.lv.float().unsqueeze(-1), v], -1)
    assert torch.equal(torch.einsum("bhdn,bhen->bhde", k.softmax(-1), v), c.want_ctx)


def test_linattn_shapes_reach_every_path():
    """The lists of the issue, by the predicates (asserted against the restatement below)."""
    for bf16 in (False, True):
        Rr = R.rows_per_trip(bf16)
        assert Rr == (64 if bf16 else 32)
        cases = [a for a in LIN_ARGS if a["bf16"] == bf16]
        paths = set().union(*(R.seg_paths(a["N"], a["nseg"], bf16) for a in cases))
        want = {"len%d" % n for n in (1, Rr - 1, Rr, Rr + 1, 63, 64, 65, 4 * Rr - 1, 4 * Rr, 4 * Rr + 1, 8 * Rr + 1)}
        want |= {"empty_segment", "shorter_than_a_load", "clamped_trip", "two_trips", "ragged_tile", "two_tiles", "ragged_last_segment",
                 "combine_second_batch", "combine_ragged_batch", "combine_third_batch"}
        assert want <= paths, sorted(want - paths)
        assert {a["nseg"] for a in cases if a["N"] == 130} >= {1, 31, 32, 33, 64, 65}
        for ns in (33, 64, 65):                  # a segment without a zero key in every batch of 32 that has a second one to carry the zero
            dead = [a["dead"] for a in cases if a["N"] == 130 and a["nseg"] == ns][0]
            live = len([1 for n0, n1 in R.segments(130, ns) if n1 > n0])
            assert all(any(32 * bt <= s < 32 * bt + 32 for s in dead) for bt in range((live + 31) // 32) if live - 32 * bt >= 2), (ns, dead)
        assert {a["heads"] for a in cases} >= {1, 4, 7, 8} and {a["B"] for a in cases} == {1, 3}
        assert any(a.get("token") and a.get("pad") for a in cases) and any(not a.get("token") for a in cases)
        outs = [a for a in cases if "q_softmax" in a]
        assert {a["N"] for a in outs} >= {1, 63, 64, 65, 255, 256, 257, 513}
        assert {(a["q_softmax"], a["lq"]) for a in outs} == {(0, False), (1, False), (1, True)}
        assert {a["heads"] for a in outs if a["q_softmax"]} >= {1, 4, 7, 8}
        op = set().union(*(R.out_paths(a["N"], bf16) for a in outs))
        assert {"two_blocks", "three_blocks", "ragged_block"} <= op and (bf16 or {"wave_without_a_row", "ragged_wave"} <= op)
        if not bf16:
            assert "wave_without_a_row" in R.out_paths(65, False)
        assert all(a["N"] <= 700 and a["B"] <= 3 and a["nseg"] <= a["N"] for a in cases)


def _brute_seg_paths(N, nseg, bf16):
    """attn_ctx_partial's loops thread by thread, attn_ctx_combine's batches."""
    V = 8 if bf16 else 4
    DV = 32 // V
    Rr = 256 // DV
    per = (N + nseg - 1) // nseg
    out, lens = set(), []
    for seg in range(nseg):
        n0 = seg * per
        n1 = min(N, n0 + per)
        trips, clamped, idle = 0, False, False
        for pl in range(Rr):
            n, t = n0 + pl, 0
            idle |= not n < n1
            while n < n1:
                t += 1
                clamped |= any(n + j * Rr > n1 - 1 for j in range(4))
                n += 4 * Rr
            trips = max(trips, t)
        tiles = [min(64, n1 - t0) for t0 in range(n0, n1, 64)]
        if not tiles:
            assert trips == 0
            out.add("empty_segment")
            continue
        lens.append(sum(tiles))
        out.add("len%d" % sum(tiles))
        out |= {name for name, on in (("shorter_than_a_load", idle), ("clamped_trip", clamped), ("two_trips", trips >= 2),
                                      ("ragged_tile", any(t < 64 for t in tiles)), ("two_tiles", len(tiles) >= 2)) if on}
    if len(set(lens)) > 1:
        out.add("ragged_last_segment")
    batches = [min(32, nseg - s0) for s0 in range(0, nseg, 32)]
    out |= {name for name, on in (("combine_second_batch", len(batches) >= 2), ("combine_third_batch", len(batches) >= 3),
                                  ("combine_ragged_batch", any(b < 32 for b in batches))) if on}
    return out


def _brute_out_paths(N, bf16):
    out = set()
    grid = (N + 255) // 256
    out |= {name for name, on in (("two_blocks", grid >= 2), ("three_blocks", grid >= 3)) if on}
    for blk in range(grid):
        rows = [blk * 256 + t < N for t in range(256)]
        if not all(rows):
            out.add("ragged_block")
        if not bf16:
            for w in range(4):
                nb = blk * 256 + 64 * w
                inside = sum(nb + r < N for r in range(64))
                if inside == 0:
                    out.add("wave_without_a_row")
                elif inside < 64:
                    out.add("ragged_wave")
    return out


def test_linattn_predicates_match_the_launch_arithmetic():
    shapes = {(a["N"], a["nseg"], a["bf16"]) for a in LIN_ARGS} | {(n, s, b) for b in (False, True) for n in (1, 2, 10, 66, 130, 257) for s in (1, 2, 7, 33) if s <= n}
    for N, nseg, bf16 in sorted(shapes):
        assert R.seg_paths(N, nseg, bf16) == _brute_seg_paths(N, nseg, bf16), (N, nseg, bf16)
    for bf16 in (False, True):
        for N in list(range(1, 70)) + [127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 512, 513, 700]:
            assert R.out_paths(N, bf16) == _brute_out_paths(N, bf16), (N, bf16)
    assert R.segments(10, 7)[5:] == [(10, 10), (12, 10)]


# (defect model, the GPU case that shows it, the compared tensor)
LIN_SHOWN = [
    ("seg_last_row_dropped", "f32_B1_N63_h8_s2", "ctx"),
    ("tile_clamp_counted", "f32_B3_N61_h4_s2_tok_pad8", "ctx"),
    ("tile_clamp_counted", "bf16_B3_N125_h4_s2_tok_pad8", "ctx"),
    ("sweep1_trip_clamp_wrong_max", "f32_B3_N253_h4_s2", "ctx"),
    ("sweep1_trip_clamp_wrong_max", "bf16_B1_N509_h4_s2", "ctx"),
    ("combine_second_batch_lost", "bf16_B3_N130_h4_s33_tok_pad8_dead1", "ctx"),
    ("combine_second_batch_lost", "f32_B3_N130_h4_s64_tok_pad8_dead1-40", "ctx"),
    ("combine_second_batch_lost", "f32_B1_N130_h1_s65_dead1-40", "ctx"),
    ("combine_ragged_batch_counted_twice", "f32_B1_N130_h1_s33_dead1", "ctx"),
    ("combine_ragged_batch_counted_twice", "bf16_B3_N130_h4_s65_tok_pad8_dead1-40", "ctx"),
    ("token_ignored", "f32_B3_N130_h4_s32_tok_pad8_dead1", "ctx"),
    ("token_ignored", "bf16_B1_N10_h1_s7_tok_pad8", "ctx"),
    ("token_stride_as_HD", "bf16_B3_N130_h4_s31_tok_pad8_dead1", "ctx"),
    ("token_stride_as_HD", "f32_B3_N257_h1_s2_tok_pad8", "ctx"),
    ("lq_stride_as_HD", "f32_B3_N1_h1_s1_pad8_qs_lq", "out"),
    ("lq_stride_as_HD", "bf16_B3_N64_h7_s2_pad8_qs_lq", "out"),
    ("k_v_offsets_swapped", "f32_B3_N10_h4_s7", "ctx"),
    ("k_v_offsets_swapped", "bf16_B1_N2_h1_s2", "ctx"),
    ("head_h_reads_head_0", "bf16_B3_N10_h4_s7", "ctx"),
    ("head_h_reads_head_0", "f32_B1_N255_h8_s2", "ctx"),
    ("out_second_block_lost", "f32_B1_N257_h4_s1", "out"),
    ("out_second_block_lost", "bf16_B1_N513_h8_s2_pad8_qs_lq", "out"),
    ("empty_segment_counted", "f32_B3_N10_h4_s7", "ctx"),
    ("empty_segment_counted", "bf16_B1_N10_h1_s7_tok_pad8", "ctx"),
]


def test_every_linattn_defect_model_is_listed():
    assert {k for k, _, _ in LIN_SHOWN} == set(R.LINATTN_MUTANTS)


@pytest.mark.parametrize("kind,a,what", LIN_SHOWN)
def test_linattn_defect_shows_in_a_gpu_case(kind, a, what):
    c = _lin(a)
    m = R.linattn_mutant(c, kind)
    assert m is not None, "the fault cannot show at this shape"
    ctx, out = m
    if what == "ctx":
        assert ctx.shape == c.want_ctx.shape and not torch.equal(ctx, c.want_ctx)
    else:
        assert out.shape == c.want_out.shape and out.dtype == c.want_out.dtype and not torch.equal(out, c.want_out)


def test_linattn_walk_without_a_fault_is_no_defect():
    c = R.linattn_case(**LIN_ARGS[3])
    assert torch.equal(R.linattn_ctx_walk(c, fault=None), c.want_ctx)


# ================================================================================================= vq_attn
def test_vq_segments_rule_values():
    assert R.vq_segments_rule(1, 657, 80) == 24 and R.vq_segments_rule(128, 8192, 80) == 16 and R.vq_segments_rule(600, 700, 160) == 4
    assert R.vq_segments_rule(9, 128 * 100, 160) == 4 * 28 and R.vq_segments_rule(2, 128 * 100, 80) == 256


@pytest.mark.parametrize("C,B,N,skip", sorted({a[:4] for a in VQ_ARGS}), ids=lambda v: str(v))
def test_vq_case_is_exact_in_any_order(C, B, N, skip):
    c = R.vq_case(C, B, N, skip)
    R.vq_preconditions(c)
    ctx64, wfold64, y64 = R.vq_ref64(c)
    assert torch.equal(ctx64.double(), c.ctx) and torch.equal(wfold64.double(), c.wfold) and torch.equal(y64.double(), c.y)
    assert not wfold64[:, C:].any()
    if skip:
        assert not torch.equal(wfold64[:, :C].double(), c.wb), "the bf16 store of the fold was to round"
    nsegs = sorted({a[4] for a in VQ_ARGS if a[:4] == (C, B, N, skip)} | {4, 4 * ((N + 127) // 128)})
    for nseg in nsegs:                                                           # every block / wave / tile order the GPU test runs, and two more
        ctx32 = R.vq_ctx_walk(c, nseg)
        assert ctx32.dtype == torch.float32 and torch.equal(ctx32, ctx64), nseg
        ctxb = R.vq_ctx_walk(c, nseg, round_pv=True)                             # P and V as bf16 matrix-core operands: nothing to round
        assert torch.equal(ctxb, ctx64), nseg
    wfold32, y32 = R.vq_out_walk(c, ctx64, nsegs[0])
    assert torch.equal(wfold32, wfold64) and torch.equal(y32, y64)
    for nseg in nsegs:
        st = R.vq_stats(y64, N, nseg)
        # fp32 running sums in two orders (forwards, backwards) of each block's pixels: equal to float64
        for i, (p0, p1) in enumerate(R.vq_block_pixels(N, nseg)):
            yy = y64[:, p0:p1].float()
            for seq in (yy, yy.flip(1)):
                s1, s2 = torch.zeros(B, C), torch.zeros(B, C)
                for r in range(seq.shape[1]):
                    s1, s2 = s1 + seq[:, r], s2 + seq[:, r] * seq[:, r]
                assert torch.equal(s1.double(), st[:, i, :, 0]) and torch.equal(s2.double(), st[:, i, :, 1])
        assert torch.equal(st.sum(1)[..., 0], y64.double().sum(1))


def _brute_vq(N, nseg):
    """The loops of vq_attn_ctx_kernel / vq_attn_apply_kernel block by block: groups walked, buffers used, prefetch targets, tiles."""
    ngroups, nblk = (N + 127) // 128, nseg // 4
    per = (ngroups + nblk - 1) // nblk
    out, pix = set(), []
    for blk in range(nblk):
        g0 = blk * per
        g1 = min(ngroups, g0 + per)
        if not g0 < g1:
            out.add("empty_block")
            pix.append((min(N, g0 * 128),) * 2)
            continue
        walked, bufs, clamps = 0, set(), set()
        loaded = [g0, g0 + 1 if g0 + 1 < g1 else g0]                             # xs.load(g0); next(sm, .., g0 + 1 or g0)
        first = None
        for g in range(g0, g1):
            walked += 1
            bufs.add((g - g0) & 1)
            for w in range(4):
                px0 = g * 128 + w * 32
                if px0 >= N:
                    out.add("wave_past_N")
                else:
                    first = px0 if first is None else first
                    last = min(N, px0 + 32)
                    if px0 + 32 > N:
                        out.add("ragged_tile")
                        if g > g0:
                            out.add("ragged_tile_in_a_later_group")
            nxt = g + 2 if g + 2 < g1 else g
            clamps.add(nxt == g)
            loaded.append(nxt)
        assert loaded[:walked] == list(range(g0, g1)), "the double buffer hands group g its own rows"
        out.add("walks%d" % walked)
        if walked >= 3:
            assert bufs == {0, 1} and clamps == {False, True}
            out.add("walks_three_or_more")
        pix.append((first, last))
    return out, pix


def test_vq_predicates_match_the_launch_arithmetic():
    for N in sorted(set(R.VQ_N) | {64, 96, 97, 256, 384, 385, 512, 513, 640, 641, 700}):
        for nseg in sorted({4, 8, 12, 16, 20, 24, 28, 4 * ((N + 127) // 128), R.vq_segments_rule(1, N, 80), R.vq_segments_rule(3, N, 160)}):
            paths, pix = _brute_vq(N, nseg)
            assert R.vq_paths(N, nseg) == paths, (N, nseg)
            assert R.vq_block_pixels(N, nseg) == pix, (N, nseg)


def test_vq_shapes_reach_every_path():
    for C in (80, 160):
        cases = [a for a in VQ_ARGS if a[0] == C]
        assert {a[2] for a in cases} >= {1, 31, 32, 33, 127, 128, 129, 257, 657}
        assert all(a[2] <= 700 and a[1] <= 3 and a[4] >= 4 and a[4] % 4 == 0 for a in cases)
        assert {a[1] for a in cases} == {1, 3} and {a[3] for a in cases} == {True, False} and {a[5] for a in cases} == {True, False}
        assert all((C, B, N, skip, R.vq_segments_rule(B, N, C)) in {a[:5] for a in cases} for _, B, N, skip, _, _ in cases[:len(R.VQ_N)])
        p657 = R.vq_paths(657, 4)
        assert "walks6" in p657 and "wave_past_N" in p657 and (C, 3, 657, True, 4, True) in cases
        assert R.vq_blocks(600, 8) == (5, [(0, 3), (3, 5)]) and "ragged_tile_in_a_later_group" in R.vq_paths(600, 8) and any(a[2:5:2] == (600, 8) for a in cases)
        assert R.vq_blocks(600, 16) == (5, [(0, 2), (2, 4), (4, 5), (6, 5)]) and "empty_block" in R.vq_paths(600, 16) and any(a[2:5:2] == (600, 16) for a in cases)
        assert any(a[4] == 4 * ((a[2] + 127) // 128) and a[2] > 512 for a in cases)
        paths = set().union(*(R.vq_paths(a[2], a[4]) for a in cases))
        assert {"walks1", "walks2", "walks3", "walks6", "walks_three_or_more", "empty_block", "wave_past_N", "ragged_tile", "ragged_tile_in_a_later_group"} <= paths
        assert any("empty_block" in R.vq_paths(a[2], a[4]) and a[5] for a in cases), "an empty block with statistics"
        assert any(not a[5] for a in cases)


def test_vq_segments_rule_is_monotone_in_the_plain_sense():
    for C in (80, 160):
        for B in (1, 2, 8, 9, 64, 128, 600):
            for N in (1, 128, 129, 700):
                ns = R.vq_segments_rule(B, N, C)
                assert 4 <= ns <= 256 and ns % 4 == 0 and ns // 4 <= max(1, (N + 127) // 128)


VQ_SHOWN = [
    ("ragged_rows_unmasked", (80, 3, 657, True, 4, True), "ctx"),
    ("ragged_rows_unmasked", (160, 1, 33, True, 4, False), "ctx"),
    ("wave_past_N_counted", (80, 1, 1, False, 4, True), "ctx"),
    ("wave_past_N_counted", (160, 3, 657, True, 4, True), "ctx"),
    ("group_parity_swapped", (80, 3, 600, True, 8, True), "y"),
    ("group_parity_swapped", (160, 3, 657, True, 4, True), "y"),
    ("third_group_stale", (80, 3, 657, True, 4, True), "ctx"),
    ("third_group_stale", (160, 3, 600, True, 8, True), "y"),
    ("empty_block_stats_stale", (80, 3, 600, True, 16, True), "stats"),
    ("empty_block_stats_stale", (160, 3, 33, True, 8, True), "stats"),
    ("wnin_dropped", (80, 3, 657, True, 4, True), "wfold"),
    ("wnin_dropped", (160, 3, 600, True, 8, True), "y"),
    ("bias_dropped", (80, 1, 1, False, 4, True), "y"),
    ("bias_dropped", (160, 3, 600, False, 16, True), "y"),
    ("fold_rows_past_C_kept", (80, 1, 1, False, 4, True), "wfold"),
    ("ctx_transposed", (80, 3, 657, True, 4, True), "wfold"),
    ("ctx_transposed", (160, 3, 600, False, 16, True), "y"),
]


def test_every_vq_defect_model_is_listed():
    assert {k for k, _, _ in VQ_SHOWN} == set(R.VQ_MUTANTS)


@pytest.mark.parametrize("kind,a,what", VQ_SHOWN, ids=lambda v: v if isinstance(v, str) else "C%d_B%d_N%d_%s_s%d_%s" % v)
def test_vq_defect_shows_in_a_gpu_case(kind, a, what):
    assert a in VQ_ARGS, "not a case of the GPU test"
    C, B, N, skip, nseg, st = a
    c = R.vq_case(C, B, N, skip)
    want = R.vq_expect(c, nseg)
    m = R.vq_mutant(c, nseg, kind)
    assert m is not None, "the fault cannot show at this shape"
    got = dict(zip(("ctx", "wfold", "y", "stats"), m))[what]
    ref = getattr(want, what)
    assert what != "stats" or st
    assert got.shape == ref.shape and not torch.equal(got.double(), ref.double())


def test_vq_walk_without_a_fault_is_no_defect():
    c = R.vq_case(80, 3, 600, True)
    want = R.vq_expect(c, 8)
    ctx = R.vq_ctx_walk(c, 8)
    wfold, y = R.vq_out_walk(c, ctx, 8)
    assert torch.equal(ctx, want.ctx) and torch.equal(wfold, want.wfold) and torch.equal(y, want.y)


# ================================================================================================= the random-data yardsticks
@pytest.mark.parametrize("a", R.LINATTN_RANDOM, ids=lambda a: "_".join(map(str, a)))
def test_linattn_restatement_is_close_to_float64(a):
    c = R.linattn_random_case(*a)
    ctx64 = R.linattn_ctx_walk(c, nseg=1, dtype=torch.float64)
    ctx32 = R.linattn_ctx_walk(c)
    e = R.row_errors(ctx32, ctx64).max().item()
    assert 0 < e < 1e-5, e
    out64, out32 = R.linattn_out_walk(c, ctx64, dtype=torch.float64), R.linattn_out_walk(c, ctx32)
    e = R.row_errors(out32, out64).max().item()
    assert 0 < e < 1e-5, e
    assert c.N <= 700 and c.B <= 3


@pytest.mark.parametrize("a", R.VQ_RANDOM, ids=lambda a: "_".join(map(str, a)))
def test_vq_restatement_is_close_to_float64(a):
    c = R.vq_random_case(*a)
    nseg = R.vq_segments_rule(c.B, c.N, c.C)
    ctx64 = R.vq_ctx_walk(c, 4, dtype=torch.float64)
    ctxb = R.vq_ctx_walk(c, nseg, round_pv=True)
    assert 0 < R.row_errors(ctxb, ctx64).max().item() < 6e-2
    _, y64 = R.vq_out_walk(c, ctx64, nseg, dtype=torch.float64)
    _, yb = R.vq_out_walk(c, ctxb, nseg)
    assert 0 < R.row_errors(yb, y64).max().item() < 6e-2
