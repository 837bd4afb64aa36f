"""CPU tests (no GPU) that pin tests/probtrack_ref.py, the NumPy restatement the GPU tests hold fibd_prob_table / fibd_prob_run to:
known answers of the generator, a hand-worked table, the sampler's distribution, straight runs, the cone, determinism, a scalar
transcription of the definition -- and the mutants of DESIGN.md §5, each of which one named check must notice."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probtrack_ref as R  # noqa: E402

F32 = np.float32


def cosd(a):
    return F32(np.cos(np.deg2rad(np.float64(a))))


# ---- generator -------------------------------------------------------------------------------------------------------------------
def test_generator_known_answers():
    assert R.h32(0, 0, 0) == 2802244911
    assert R.h32(1234, 5, 2) == 1460108722
    assert R.h32(2 ** 63 + 1, 10 ** 6, 141) == 2790284181
    rng = np.random.default_rng(0)
    lines, ks = rng.integers(0, 2 ** 40, 200), rng.integers(0, 300, 200)
    for seed in (0, 1234, 2 ** 63 + 1, 2 ** 64 - 1):
        assert [int(x) for x in R.h32_v(seed, lines, ks)] == [R.h32(seed, int(a), int(b)) for a, b in zip(lines, ks)]


# ---- table -----------------------------------------------------------------------------------------------------------------------
def test_table_hand_worked_rows():
    nan, inf = np.nan, np.inf
    rows = np.array([[1, 2, 3, 5],            # 0 plain
                     [nan, 2, 4, 3],          # 1 a NaN
                     [-inf, 1, 2, 3],         # 2 -Inf
                     [1, inf, 2, 3],          # 3 +Inf
                     [2, 2, 2, 2],            # 4 constant
                     [-4, -1, -2, -3],        # 5 all negative
                     [1, 2, 3, 5],            # 6 masked
                     [nan, nan, nan, nan]],   # 7 all NaN
                    F32)
    mask = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    t = R.table(rows.T, mask, subtract_min=True, pmf_thresh=0.25)
    assert t.shape == (8, 64) and t.dtype == np.uint16 and not t[:, 4:].any()
    # w = (0, 1, 2, 4), t = (0, .25, .5, 1): the value exactly AT the threshold stays; floor(.25 * 65535) = 16383, floor(.5 * 65535) = 32767
    assert t[0, :4].tolist() == [0, 16383, 32767, 65535]
    assert t[1, :4].tolist() == [0, 0, 65535, 32767]         # m = 2 (the NaN dropped); the NaN itself becomes 0
    assert not t[2].any() and not t[3].any()                 # wmax = Inf
    assert not t[4].any()                                    # wmax = 0
    assert t[5, :4].tolist() == [0, 65535, 43690, 21845]     # w = (0, 3, 2, 1): floor(2/3 * 65535) = 43690, floor(1/3 * 65535) = 21845
    assert not t[6].any() and not t[7].any()
    u = R.table(rows.T, mask, subtract_min=False, pmf_thresh=0.25)
    # t = (.2, .4, .6, 1) as float32: .2 is below the threshold; float32(.4) * 65535 = 26214.0008 -> 26214, float32(.6) * 65535 -> 39321
    assert u[0, :4].tolist() == [0, 26214, 39321, 65535]
    assert u[1, :4].tolist() == [0, 32767, 65535, 49151]     # (0, .5, 1, .75)
    assert u[2, :4].tolist() == [0, 21845, 43690, 65535]     # -Inf is clipped to 0 like any negative value
    assert not u[3].any()
    assert u[4, :4].tolist() == [65535] * 4
    assert not u[5].any() and not u[6].any() and not u[7].any()
    assert np.array_equal(R.table(rows.T, None, True, 0.25)[6], t[0])


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvert,rng_seed,k", [(181, 1234, 0), (321, 7, 3), (362, 99, 1)])
def test_sampler_distribution(nvert, rng_seed, k):
    rng = np.random.default_rng(5)
    q = np.floor(rng.random(nvert) ** 4 * 65535).astype(np.int64)
    q[rng.random(nvert) < 0.4] = 0
    N = 200000
    u = R.h32_v(rng_seed, np.arange(N), np.full(N, k))
    pick = R.draw(np.broadcast_to(q, (N, nvert)), u)
    n = np.bincount(pick, minlength=nvert)
    assert not n[q == 0].any(), "a vertex of zero weight was picked"
    e = N * q / q.sum()
    big = e >= 5
    obs, exp = list(n[big]), list(e[big])
    if (~big & (q > 0)).any():                                   # cells with an expectation below 5, pooled
        obs.append(n[~big].sum()); exp.append(e[~big].sum())
    obs, exp = np.array(obs, np.float64), np.array(exp, np.float64)
    chi2, df = ((obs - exp) ** 2 / exp).sum(), obs.size - 1
    print("chi2 %.1f df %d z %.2f" % (chi2, df, (chi2 - df) / np.sqrt(2 * df)))
    assert chi2 <= df + 5 * np.sqrt(2 * df)


# ---- the checks the mutants are run against ------------------------------------------------------------------------------------------
def check_step_rounding(mutant=None):
    """nxt = pos + vec * step with TWO roundings: the product of two float32 is exact in float64, and so is the sum of two float32 of
    this range, so float64 arithmetic rounded to float32 after each operation is the hand calculation"""
    rng = np.random.default_rng(0)
    pos = rng.uniform(1, 12, (4000, 3)).astype(F32)
    vec = rng.uniform(-1, 1, (4000, 3)).astype(F32)
    step = F32(0.3)
    prod = (vec.astype(np.float64) * np.float64(step)).astype(F32)
    want = (pos.astype(np.float64) + prod.astype(np.float64)).astype(F32)
    fused = (pos.astype(np.float64) + vec.astype(np.float64) * np.float64(step)).astype(F32)
    assert (want != fused).sum() > 100                          # (the inputs tell the two apart)
    assert np.array_equal(R.step_point(pos, vec, step, mutant), want)


def _axis_field():
    """8 x 3 x 3 voxels, U = the axes; the voxels with 2 <= x <= 6 (1-based) hold vertex 0 only, the others nothing"""
    U = np.eye(3, dtype=F32)
    shape = (8, 3, 3)
    tab = np.zeros((8 * 3 * 3, 64), np.uint16)
    lin = np.arange(72)
    x = lin % 8 + 1
    tab[(x >= 2) & (x <= 6), 0] = 40000
    seeds = np.array([2 + 8 * (1 + 3 * 1), 2 + 8 * (0 + 3 * 2)], np.int64)      # x = 3 (1-based)
    return U, shape, tab, seeds


def check_straight_runs(mutant=None):
    U, shape, tab, seeds = _axis_field()
    sub = np.zeros((1, 3), F32)
    r = R.trace(tab, U, cosd(45), shape, seeds, sub, len_min=1, len_max=40, step_size=0.5, rng_seed=3, mutant=mutant)
    # forward: 3.5 -> voxel 4 (tie to even), 4.5 -> 4, 5.5 -> 6, 6.5 -> 6, 7.0 -> 7 which is empty: the points 3 .. 6 are saved, 7 of them;
    # backward: 2.5 -> 2, 2.0, 1.5 -> 2, 1.0 -> voxel 1 which is empty: 3, 2.5, 2 are saved
    assert r["npts"].tolist() == [10, 10] and r["all_counts"].tolist() == [[7, 3], [7, 3]]
    want_x = [6.0, 5.5, 5.0, 4.5, 4.0, 3.5, 3.0, 3.0, 2.5, 2.0]                 # the seed twice
    xyz = r["xyz"].reshape(2, 10, 3)
    assert xyz[0, :, 0].tolist() == want_x and xyz[1, :, 0].tolist() == want_x
    assert (xyz[0, :, 1:] == [2, 2]).all() and (xyz[1, :, 1:] == [1, 3]).all()
    # the cap: forward ends when npts = len_max + 1, backward adds one
    r = R.trace(tab, U, cosd(45), shape, seeds, sub, len_min=1, len_max=4, step_size=0.5, rng_seed=3, mutant=mutant)
    assert r["npts"].tolist() == [6, 6] and r["all_counts"].tolist() == [[5, 1], [5, 1]]
    assert r["xyz"].reshape(2, 6, 3)[0, :, 0].tolist() == [5.0, 4.5, 4.0, 3.5, 3.0, 3.0]
    # len_min drops, the order of the rest stays
    r = R.trace(tab, U, cosd(45), shape, seeds, sub, len_min=11, len_max=40, step_size=0.5, rng_seed=3, mutant=mutant)
    assert r["npts"].size == 0 and r["xyz"].shape == (0, 3)


def check_cone_boundary(mutant=None):
    U = np.array([[1, 0, 0], [0.5, np.sqrt(0.75), 0], [0, 0, 1]], F32)
    allow, same = R.cone(U, 0.5, mutant)                        # c(0, 1) = 1 * .5 + 0 + 0 = .5 exactly
    assert allow[0, 1] and allow[1, 0] and not allow[0, 2] and allow[2, 2]
    assert same[0, 1] and not same[0, 2]


def _random_field(seed=11, shape=(6, 5, 4), zero_frac=0.15):
    import fibers_jl_amd as fj
    U = np.ascontiguousarray(fj.sphere_362.vertices[:181], F32)
    rng = np.random.default_rng(seed)
    nvox = shape[0] * shape[1] * shape[2]
    tab = np.zeros((nvox, 192), np.uint16)
    tab[:, :181] = np.floor(rng.random((nvox, 181)) ** 4 * 65535)
    tab[rng.random(nvox) < zero_frac] = 0
    seeds = np.arange(nvox, dtype=np.int64)
    sub = rng.uniform(-0.49, 0.49, (2, 3)).astype(F32)
    return U, shape, tab, seeds, sub


def check_cone_angles(mutant=None):
    """no two successive segments of a line make an angle above ang_thresh.  The cone is defined on c(j, i) = |U_j| |U_i| cos(angle), and the
    sphere tables are unit vectors to 3-4 digits only (norms 0.9994 .. 1.0005), so what the definition promises is
    cos(angle) >= cosang_thresh / max|U|^2.  A segment is the difference of two float32 positions below 16, each within 2^-21 of its exact
    value, and is 0.5 long: its direction is off by < 1e-5, the tolerance is 1e-4 on the cosine."""
    U, shape, tab, seeds, sub = _random_field()
    nmax2 = (np.linalg.norm(U.astype(np.float64), axis=1) ** 2).max()
    for ang in (20, 45, 80):
        r = R.trace(tab, U, cosd(ang), shape, seeds, sub, len_min=3, len_max=12, step_size=0.5, rng_seed=ang, mutant=mutant)
        assert r["npts"].size > 20
        off = np.concatenate([[0], np.cumsum(r["npts"])])
        worst = 1.0
        for a, b in zip(off[:-1], off[1:]):
            seg = np.diff(r["xyz"][a:b].astype(np.float64), axis=0)
            seg = seg[np.linalg.norm(seg, axis=1) > 0]            # (the seed is there twice)
            seg /= np.linalg.norm(seg, axis=1)[:, None]
            if len(seg) > 1:
                worst = min(worst, (seg[:-1] * seg[1:]).sum(axis=1).min())
        assert worst >= np.cos(np.deg2rad(ang)) / nmax2 - 1e-4, (ang, worst)


def _scalar_trace(tab, U, thresh, shape, seeds, sublist, len_min, len_max, step, rng_seed):
    """the definition, transcribed line by line and draw by draw (Python integers, float32 scalars)"""
    nx, ny, nz = shape
    nvert, nsub = U.shape[0], sublist.shape[0]
    step, thresh = F32(step), F32(thresh)

    def c(j, i):
        return F32(F32(F32(U[j, 0] * U[i, 0]) + F32(U[j, 1] * U[i, 1])) + F32(U[j, 2] * U[i, 2]))

    def pick(q, line, k):
        Q = sum(q)
        r = (R.h32(rng_seed, line, k) * Q) >> 32
        run = 0
        for i, w in enumerate(q):
            run += w
            if run > r:
                return i

    npts_out, sidx, xyz = [], [], []
    for line in range(len(seeds) * nsub):
        sd, sub = int(seeds[line // nsub]), line % nsub
        pos0 = [F32(F32(v + 1) + sublist[sub, a]) for a, v in enumerate((sd % nx, (sd // nx) % ny, sd // (nx * ny)))]
        row = [int(w) for w in tab[sd, :nvert]]
        fwd, bwd, npts, k = [], [], 0, 0
        if sum(row) > 0:
            j0 = pick(row, line, k)
            k += 1
            for s0, dst in ((F32(1), fwd), (F32(-1), bwd)):
                pos, j, s = list(pos0), j0, s0
                while True:
                    nxt = [F32(pos[a] + F32(F32(s * U[j, a]) * step)) for a in range(3)]
                    if not all(np.isfinite(nxt)):
                        break
                    v = [int(np.rint(x)) for x in nxt]
                    if not (1 <= v[0] <= nx and 1 <= v[1] <= ny and 1 <= v[2] <= nz):
                        break
                    lin = (v[0] - 1) + nx * ((v[1] - 1) + ny * (v[2] - 1))
                    q = [int(tab[lin, i]) if abs(c(j, i)) >= thresh else 0 for i in range(nvert)]
                    if sum(q) == 0:
                        break
                    i = pick(q, line, k)
                    k += 1
                    if not c(j, i) > 0:
                        s = -s
                    j = i
                    dst.append(pos)
                    npts += 1
                    if npts > len_max:
                        break
                    pos = nxt
        if npts >= len_min:
            npts_out.append(npts); sidx.append(line); xyz += fwd[::-1] + bwd
    return np.array(npts_out, np.int32), np.array(sidx, np.int64), np.array(xyz, F32).reshape(-1, 3)


_scalar_cache = {}


def check_against_scalar(mutant=None):
    U, shape, tab, seeds, sub = _random_field(seed=4, shape=(4, 3, 3), zero_frac=0.3)
    U = U[:40]
    args = (tab, U, cosd(60), shape, seeds, sub, 2, 4, 0.5, 77)
    if "want" not in _scalar_cache:
        _scalar_cache["want"] = _scalar_trace(*args)
    npts, sidx, xyz = _scalar_cache["want"]
    assert npts.size > 10 and (npts < 6).any() and npts.max() == 6          # lines that end on their own, and the cap
    r = R.trace(*args[:6], len_min=2, len_max=4, step_size=0.5, rng_seed=77, mutant=mutant)
    assert np.array_equal(r["npts"], npts) and np.array_equal(r["seed_index"], sidx)
    assert r["xyz"].tobytes() == xyz.tobytes()


CHECKS = {"fma": check_step_rounding, "floor": check_straight_runs, "draw_first": check_against_scalar, "allow_gt": check_cone_boundary,
          "same_row": check_cone_angles}


@pytest.mark.parametrize("check", sorted(set(CHECKS.values()), key=lambda f: f.__name__), ids=lambda f: f.__name__)
def test_restatement(check):
    check()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_noticed(mutant):
    """the check named for a mutant fails on it; the scalar transcription notices every mutant that changes a line"""
    with pytest.raises(AssertionError):
        CHECKS[mutant](mutant)
    if mutant in ("draw_first", "same_row"):                     # (0.5 * U is exact, no coordinate is a tie and no c(j, i) equals cosd(60) there)
        with pytest.raises(AssertionError):
            check_against_scalar(mutant)


def test_same_arguments_same_bytes_other_seed_other_lines():
    U, shape, tab, seeds, sub = _random_field()
    a = R.trace(tab, U, cosd(45), shape, seeds, sub, rng_seed=5)
    b = R.trace(tab, U, cosd(45), shape, seeds, sub, rng_seed=5)
    c = R.trace(tab, U, cosd(45), shape, seeds, sub, rng_seed=6)
    for k in ("npts", "seed_index", "xyz"):
        assert a[k].tobytes() == b[k].tobytes()
    assert a["xyz"].tobytes() != c["xyz"].tobytes()
    # seeds on a zero row or outside the volume have no points, and do not disturb the others' numbering
    zero = int(np.flatnonzero(~tab.any(axis=1))[0])
    d = R.trace(tab, U, cosd(45), shape, np.array([zero, -1, tab.shape[0], 7], np.int64), sub, len_min=0, rng_seed=5)
    assert d["all_counts"][:6].sum() == 0 and d["npts"][:6].tolist() == [0] * 6 and d["seed_index"].tolist() == list(range(8))


def test_ang_thresh_90_is_refused():
    U, shape, tab, seeds, sub = _random_field()
    with pytest.raises(ValueError):
        R.trace(tab, U, F32(0.0), shape, seeds, sub)
    with pytest.raises(ValueError):
        R.trace(tab, U, F32(-0.5), shape, seeds, sub)
