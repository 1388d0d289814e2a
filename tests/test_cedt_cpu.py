"""The CPU side of the CELossDT weight-map tests: tests/cedt_ref.py (reference, checker, case builders) held to a brute-force
transform, to oracle/ref_cpu.py, and to the conditions its cases promise.  No GPU, no library."""
import numpy as np
import pytest

from tests import cedt_ref as R

SIGMA = R.GEOMETRY_SIGMA
_BRUTE = [n for n in R.GEOMETRY if n not in R.WIDE]


def test_k_res_is_computed_from_the_table():
    """The zone in which one ulp of weight pins D^2: 148 px at sigma = 5, 257 px at 7.5, about 270 px at the largest sigma."""
    assert R.k_res(5.0) == 22038 and R.k_res(7.5) == 66189
    assert 270.0 ** 2 < R.k_res(7.8) < 271.0 ** 2
    for s in (0.5, 1.0, 5.0, 7.5, 7.8):
        t = R.tab(s).astype(np.float64)
        assert ((t[:R.k_res(s)] - t[1:R.k_res(s) + 1]) >= 3 * R.ULP).all()
        assert R.k_res(s) < R.k_cut(s) and (R.tab(s)[R.k_cut(s):] == 1.0).all() and R.tab(s)[0] == 2.0


def test_the_cut_off_is_far_from_a_rounding_tie():
    """check() wants 1.0f exactly where the reference is 1.0f and nowhere else.  exp(-d / sigma^2) + 1 rounds to 1.0f iff
    exp(..) <= 2^-24; the last entry above and the first one below miss that tie by 1e-6 (relative) or more, ten orders more
    than two double evaluations differ by -- also with 1 / sigma^2 multiplied in, and with sigma rounded to float32 (7.8)."""
    for s in (0.5, 1.0, 5.0, 7.5, 7.8):
        kc = R.k_cut(s)
        for sig in (s, float(np.float32(s))):
            e = np.exp(-np.sqrt(np.array([kc - 1.0, kc])) * (1.0 / (sig * sig))) * 2.0 ** 24
            assert e[0] - 1 > 1e-6 and 1 - e[1] > 1e-6, (s, sig, e)
        # the kernel's table ((16.64 sigma^2 + 2)^2 entries, 1.0f beyond) ends past the cut-off
        assert int((16.64 * s * s + 2.0) ** 2) >= kc


@pytest.mark.parametrize("name", _BRUTE)
def test_scipy_squared_distance_equals_brute_force(name):
    t, k = R.case(name)
    assert t.shape[1] * t.shape[2] ** 2 <= R.BRUTE_BUDGET
    assert np.array_equal(R.brute_k(R.boundary(t)), k)


def test_brute_force_budget_leaves_out_only_the_wide_rows():
    for n in R.WIDE:
        t, _ = R.case(n)
        assert t.shape[1] * t.shape[2] ** 2 > R.BRUTE_BUDGET
    for t in (R.left_blob(3, 600), R.existing_97()):
        bd = R.boundary(t)
        assert np.array_equal(R.brute_k(bd), R.k_ref(bd))


def test_boundary_restatement_matches_the_oracle():
    """oracle.ref_cpu.cedt_weight is 2.0f = tab[0] exactly on its boundary and below 2 everywhere else."""
    import torch
    from oracle import ref_cpu
    from tests.golden.cases import cedt_cases
    for tgt, _ in cedt_cases():
        w = ref_cpu.cedt_weight(tgt, 5.0).numpy()
        assert np.array_equal(w == R.tab(5.0)[0], R.boundary(tgt.numpy()))
        R.check(w, tgt.numpy(), 5.0)
    for name in ("seam-5x509", "tall-341x70-s1", "tiny-1x9"):
        t, _ = R.case(name)
        w = ref_cpu.cedt_weight(torch.from_numpy(t.copy()), SIGMA).numpy()
        assert np.array_equal(w == 2.0, R.boundary(t))
        assert R.check(w, t, SIGMA) == (0.0, 1.0)


@pytest.mark.parametrize("name", list(R.GEOMETRY))
def test_every_pixel_of_a_geometry_case_is_resolvable(name):
    """The condition under which the GPU test of the case holds EVERY pixel to an exact D^2."""
    t, k = R.case(name)
    assert k.max() < R.k_res(SIGMA), (k.max(), R.k_res(SIGMA))
    assert (t == 1).any() and (t == 255).any() or name.startswith("tiny")


def test_col_plan_thresholds():
    """The heights of the tall cases sit on both sides of every threshold of the strip rule."""
    assert R.col_plan(341)[3] <= 64 * 1024 < R.col_plan(342)[3]                   # the LDS opt-in
    assert [R.col_plan(H)[:2] for H in (832, 833, 1664, 1665, 3328, 3329, 6656, 6657, 13312, 13313, 16384)] == \
        [(64, 4), (32, 8), (32, 8), (16, 16), (16, 16), (8, 32), (8, 32), (4, 64), (4, 64), (2, 128), (2, 128)]
    assert all(R.col_plan(H)[3] <= 156 * 1024 for H in range(1, 16385, 7))
    assert 72 * 1024 < R.col_plan(401)[3] and R.col_plan(500)[3] <= 96 * 1024     # the workload's own heights
    assert R.col_plan(13313)[2] * 127 > 13313                                      # its last segment has no row at all


@pytest.mark.parametrize("name", list(R.TALL))
def test_tall_cases_have_an_empty_segment_between_two_occupied_ones(name):
    t, _ = R.case(name)
    cols = R.col_plan(t.shape[1])[0]
    assert t.shape[2] % cols != 0                    # a last strip with nc < cols (W = 5 below 64 columns: the only strip)
    for b in R.boundary(t):
        assert R.empty_segments(b)


def test_tiny_and_seam_cases_hold_what_they_promise():
    for (H, W), name in zip(R.TINY_HW, R.TINY):
        t, _ = R.case(name)
        assert t.shape == (3, H, W) and (t[0] == 1).all() and 0 < (t[1:] == 1).sum() < 2 * H * W
    for W, name in zip(R.SEAM_W, R.SEAM):
        t, _ = R.case(name)
        want = [x for x in (*range(252, 257), *range(506, 511)) if x < W]
        assert sorted(set(np.nonzero(t == 1)[2])) == want
    t, _ = R.case("mixed-batch-40x57")
    bd = R.boundary(t)
    ring = np.ones((40, 57), dtype=bool)
    ring[1:-1, 1:-1] = False
    assert not bd[0].any() and np.array_equal(bd[1], ring) and bd[2].any()
    for name in R.WIDE:
        t, _ = R.case(name)
        xs = np.unique(np.nonzero(R.boundary(t))[2])
        assert np.diff(xs).max() <= 401 and xs[0] <= 100 and xs[-1] == t.shape[2] - 1


def test_the_far_case_is_exact_only_near_the_blob():
    """3 x 4097 with one blob at the left end: outside the every-pixel condition.  Only the first ~257 columns are held to an
    exact D^2; from 936 px on the weight is 1.0f and says nothing about the distance but that it is past the cut-off."""
    t = R.left_blob(3, 4097)
    k = R.k_ref(R.boundary(t))
    worst, share = R.check(R.weight_of(k, SIGMA), t, SIGMA, k)
    assert worst == 0.0 and 0.06 < share < 0.07
    assert (k >= R.k_cut(SIGMA)).mean() > 0.75


def _weak(got, ref):
    """The comparison of the tests that were here before."""
    return bool(np.allclose(got, ref, rtol=1e-6, atol=1e-6))


def _rejects(got, t, sigma, k):
    with pytest.raises(AssertionError):
        R.check(got, t, sigma, k)
    return True


def test_the_checker_rejects_wrong_distances():
    """Weights rebuilt from a corrupted D^2 must not pass check().  Whether allclose(rtol=1e-6, atol=1e-6), the comparison
    of the earlier tests, sees the same corruption (asserted below, so this record stays true):

      (a) D^2 + 1 at the single farthest pixel of tall-833x70-s2 (k = 34425, 186 px)        check fails   allclose PASSES
      (b) the rows of one empty segment of one column one row farther (carry-in off by one)   check fails   allclose fails
      (c) one column's vertical distances replaced by "no boundary"                           check fails   allclose fails
      (d) 1.0f one entry early at the cut-off (3 x 600, sigma = 5, the last pixel short of it) check fails   allclose PASSES
          and one entry late (1.0f + 1 ulp on the first pixel past it)                        check fails   allclose PASSES

    A whole row of distance, (b) and (c), is visible to both anywhere inside the zone; what the earlier comparison cannot
    see is an error of a few units in D^2 away from the boundary (a wrong candidate column, a scan that stops one round
    early): one unit of D^2 at 186 px and sigma = 7.5 moves the weight by 15 ulp, the earlier tolerance is 17 ulp and more
    (at sigma = 5, which those tests use, the same holds from about 110 px on).
    """
    name = "tall-833x70-s2"
    t, k = R.case(name)
    ref = R.weight_of(k, SIGMA)
    assert R.check(ref, t, SIGMA, k) == (0.0, 1.0)

    # (a)
    ka = k.copy()
    at = np.unravel_index(int(k.argmax()), k.shape)
    ka[at] += 1
    assert _rejects(R.weight_of(ka, SIGMA), t, SIGMA, k) and _weak(R.weight_of(ka, SIGMA), ref)

    # (b) and (c) go through the two passes of the brute-force transform, which equals k (tested above)
    bd = R.boundary(t)
    _, _, hs, _ = R.col_plan(t.shape[1])
    s, c = R.empty_segments(bd[1])[0]
    g = R.col_dist(bd[1])
    assert np.array_equal(R.row_min(g), k[1])
    gb = g.copy()
    gb[s * hs:(s + 1) * hs, c] += 1
    kb = k.copy()
    kb[1] = R.row_min(gb)
    assert (kb != k).any() and np.array_equal(kb[1, :s * hs], k[1, :s * hs]) and np.array_equal(kb[1, (s + 1) * hs:], k[1, (s + 1) * hs:])
    assert _rejects(R.weight_of(kb, SIGMA), t, SIGMA, k) and not _weak(R.weight_of(kb, SIGMA), ref)

    gc = g.copy()
    c_near = int(np.argmax(bd[1].sum(axis=0)))
    gc[:, c_near] = g.max() + (1 << 20)
    kc = k.copy()
    kc[1] = R.row_min(gc)
    assert _rejects(R.weight_of(kc, SIGMA), t, SIGMA, k) and not _weak(R.weight_of(kc, SIGMA), ref)

    # (d)
    t = R.left_blob(3, 600)
    k = R.k_ref(R.boundary(t))
    ref = R.weight_of(k, 5.0)
    assert k.max() > R.k_cut(5.0) > k[k < R.k_cut(5.0)].max() > 415 ** 2 - 1
    assert R.check(ref, t, 5.0, k)[0] == 0.0
    got = ref.copy()
    got[k == k[k < R.k_cut(5.0)].max()] = 1.0
    assert _rejects(got, t, 5.0, k) and _weak(got, ref)
    got = ref.copy()
    got[k == k[k >= R.k_cut(5.0)].min()] = np.float32(1.0 + R.ULP)          # and one entry late
    assert _rejects(got, t, 5.0, k) and _weak(got, ref)
