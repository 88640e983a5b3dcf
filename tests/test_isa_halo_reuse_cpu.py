"""The split-precision halo kernels' K loops, checked on the emitted ISA like tests/test_isa_schedule_cpu.py checks the bf16 ones (same
checker functions, no GPU needed; confined to LDS reads, LDS writes, waits and barriers).

conv3x3_halo3_hp.hip: a source chunk is 27 steps — the hi pair interleaved by tap, then the lo chunk.  A (tap, W_hi) step keeps its
pixel fragments for the (tap, W_lo) step and prefetches six weight fragments only, so its counted wait is lgkmcnt(6); every other step
prefetches ten.  Each step is held to ITS OWN count: an LDS write in the step, nothing but that many reads behind the last write.
conv_quad_halo3_split.hip: three chunks of four steps per source chunk, ten reads in every step."""
import os
import re

import pytest

from test_isa_schedule_cpu import HIPCC, _isa, _steps, _violations

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_every_split_precision_3x3_step_waits_for_its_own_read_count():
    steps = _steps(_isa("conv3x3_halo3_hp.hip"))
    assert len(steps) == 4, sorted(steps)                      # three tile widths + the two-samples-per-block form
    for kern, segs in steps.items():
        counts = [int(ops[-1][1:]) for ops in segs]
        assert set(counts) == {6, 10}, (kern, counts)
        # the loop body is ONE source chunk: nine six-read steps (one per tap of the pair), eighteen ten-read steps
        assert counts.count(6) == 9 and counts.count(10) == 18, (kern, counts)
        for ops, n in zip(segs, counts):
            assert _violations({kern: [ops]}, n) == []
            body = ops[:-1]
            after = body[len(body) - body[::-1].index("W"):]
            assert len(after) == n, (kern, "".join(o[0] for o in ops))      # not one read more than the step prefetches


@needs_hipcc
def test_split_precision_quad_steps_keep_the_ten_read_protocol():
    steps = _steps(_isa("conv_quad_halo3_split.hip"))
    assert len(steps) == 3, sorted(steps)
    for kern, segs in steps.items():
        assert len(segs) >= 12, (kern, len(segs))               # hi with W_hi, hi with W_lo, lo with W_hi: 3 x 4 steps
    assert _violations(steps, 10) == []


@needs_hipcc
@pytest.mark.parametrize("src,scratch_max", [("conv3x3_halo3_hp.hip", (0, 0, 0, 0)), ("conv_quad_halo3_split.hip", (0, 0, 40))])
def test_split_precision_halo_kernels_do_not_spill(src, scratch_max):
    """Zero scratch in the 256-register budget (the 8-wide Down / Upsample instantiation: the 40 bytes its bf16 sibling is pinned at)."""
    isa = _isa(src)
    names = re.findall(r"\.amdhsa_kernel (\S+)", isa)
    sizes = [int(x) for x in re.findall(r"; ScratchSize: (\d+)", isa)]
    vgprs = [int(x) for x in re.findall(r"; NumVgprs: (\d+)", isa)]
    assert len(names) == len(sizes) == len(vgprs) == len(scratch_max), names
    order = sorted(range(len(names)), key=lambda i: -int(re.search(r"ILi(\d)", names[i]).group(1)))      # widest tile first
    assert [sizes[i] <= scratch_max[k] for k, i in enumerate(order)] == [True] * len(order), list(zip(names, sizes))
    assert all(v <= 256 for v in vgprs), vgprs
    assert "v_pk_fma_f32" not in isa and "v_pk_add_f32" not in isa and "v_pk_mul_f32" not in isa
