"""The inputs of tests/test_hip_gn_partials.py can tell a wrong reduction of GroupNorm partials from a right one (no GPU needed).

For every consumer case of that file: the float64 reference of the consumer's operation, and the same operation with the
statistics six faulty reducers would produce (gn_partials_ref.mutant_ab: another sample's statistics, a lost tail beyond 256 or 64
partials, a lost last / first partial, one partial too many).  Each applicable fault must move the result by at least 10x the
tolerance the GPU test applies to that case — a condition on the INPUTS (distinct samples, quarter-sized end chunks), so that a
kernel with one of these faults cannot pass.  The whole-U-Net tests cannot see them: with every sample drawn from one distribution
another sample's statistics shift the result by 2e-3 .. 7e-3, below the bf16 tolerance."""
import pytest
import torch

import gn_partials_ref as R
from conftest import rel_errs


def rel_err(a, b):
    """Both error norms of the suite, the larger one — without conftest.rel_err's log: the figures here are deliberate faults, not parity."""
    return max(rel_errs(a, b))


CASES = list(R.all_cases())


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_fault_moves_the_result_ten_tolerances(case):
    # (the 64-sample grid-cap case: its samples repeat five (scale, offset) pairs, so the first five samples — each mutated with the
    # statistics the fault gives it in the whole batch — stand for all of them)
    sub = slice(0, 5) if case.stored.shape[0] > 5 else None
    for parts in case.parts:
        part = R.case_partials(case, parts)
        ab = R.ab_from_partials(part, case.count)
        # fp32 partials are not the limiting error: they give the direct float64 statistics of the stored tensor
        direct = R.ab_direct(R.nhwc(case.stored))
        assert ((ab - direct).abs() / direct.abs()).max().item() < 1e-5
        assert R.order_independent(part, case.count), (case.id, parts)
        if case.kind == "conv":
            ref, fn = case.ref_linear(ab), case.ref_linear
            if parts == case.parts[0]:
                assert rel_err(ref, case.ref(ab)) < 1e-12       # the linear form used for the mutants IS the operation
        elif sub is not None:
            fn = lambda s: case.ref(s, sub)
            ref = fn(ab)
        else:
            ref, fn = case.ref(ab), case.ref
        assert torch.isfinite(ref).all()
        seen = 0
        for kind in R.MUTANTS:
            mab = R.mutant_ab(part, case.count, kind)
            if mab is None:
                continue
            seen += 1
            moved = rel_err(fn(mab), ref)
            assert moved >= 10 * case.tol, (case.id, parts, kind, moved, case.tol)
        assert seen >= (2 if parts == 1 else 4)


def test_partials_layout():
    """make_partials: parts chunks that tile the sample, first and last about a quarter; guarded() is exercised on the GPU."""
    for n in (320, 4290, 49152):
        for parts in (1, 2, 3, 64, 65, 256, 257, 300):
            b = R.chunk_bounds(n, parts)
            assert len(b) == parts + 1 and b[0] == 0 and b[-1] == n and all(b[i] <= b[i + 1] for i in range(parts))
            if parts >= 3:
                assert abs(b[1] - n / 4) <= 1 and abs(n - b[-2] - n / 4) <= 1
    x = R.distinct_samples("gp_layout", (3, 8, 5, 7))
    p = R.make_partials(x, 65)
    s = p.double().sum(1)
    assert torch.allclose(s[:, 0], x.double().flatten(1).sum(1), rtol=1e-6) and torch.allclose(s[:, 1], (x.double() ** 2).flatten(1).sum(1), rtol=1e-6)
    assert (x.flatten(1).mean(1).abs() / x.flatten(1).std(1)).max().item() <= 3.0
