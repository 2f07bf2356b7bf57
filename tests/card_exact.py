"""The cardinality projection as a contract (pure numpy, no GPU), and the route of the engine's search restated.

`check_card_output` is an independent statement of src/projectors/project_cardinality!.jl:3-21 (stable sortperm by abs,
descending; everything behind the k-th place is zeroed): keep the k entries of largest magnitude, among equal magnitudes the
lowest indices win.  Zeros compare by value: the reference writes +0.0 over a dropped entry and leaves a kept -0.0 alone,
which of the two an engine hands back for an entry that is zero either way is not part of the contract.

`predict_route` restates the decision rule of k_card_decide (csrc/kernels_proj.hip) the way cold_bracket of
tests/test_gpu_l1_exact.py restates decide_body: which exit a search takes, how many gated refinement passes run, the final
bracket (lo, hi] and how many magnitudes the compaction gathers from it.  `inputs` builds the named vectors the CPU and GPU
tests share."""
import numpy as np

CAP = 8192                    # CARD_CAP
REFINES = 5                   # CARD_REFINES
WARM = (0.5, 0.9, 0.99, 0.999, 1.001, 1.01, 1.1, 2.0)      # k_card_select: the next search probes tau_prev * these


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_card_output(v, y, k):
    """Raise AssertionError unless y is the stable selection of the k largest magnitudes of v.  The message names the first
    offending index and which of the four rules broke: (1) y[i] is v[i] bit for bit or zero, (2) min(k, nnz) non-zeros are
    kept, (3) every kept magnitude >= every dropped one, (4) among the entries equal to tau the kept indices come first."""
    v, y = np.asarray(v), np.asarray(y)
    assert y.dtype == v.dtype and y.shape == v.shape and v.ndim == 1, "output of another type or shape"
    k = int(k)
    a = np.abs(v)
    same = _bits(v) == _bits(y)
    bad = np.nonzero(~same & (y != 0))[0]                 # (a zero of either sign is a zero)
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"rule 1 (y[i] is v[i] bit for bit, or zero) broke at index {i}: v {v[i]!r}, y {y[i]!r} ({len(bad)} entries)")
    kept = y != 0
    dropped = (v != 0) & ~kept
    nnz = int((v != 0).sum())
    want = min(max(k, 0), nnz)
    if int(kept.sum()) != want:
        # the first index at which the running count of kept entries leaves what the stable selection keeps
        ref = np.zeros(len(v), bool)
        ref[np.argsort(-a, kind="stable")[:max(k, 0)]] = True
        ref &= v != 0
        i = int(np.nonzero(ref != kept)[0][0])
        raise AssertionError(f"rule 2 (min(k, nnz) = {want} non-zeros are kept) broke: {int(kept.sum())} kept, first difference at index {i}: "
                             f"v {v[i]!r}, y {y[i]!r}")
    if not kept.any() or not dropped.any():
        return
    tau, top = a[kept].min(), a[dropped].max()
    if top > tau:
        i = int(np.nonzero((dropped & (a > tau)) | (kept & (a < top)))[0][0])
        raise AssertionError(f"rule 3 (every kept magnitude >= every dropped one) broke at index {i}: |v| {a[i]!r} was "
                             f"{'kept' if kept[i] else 'dropped'}; smallest kept {tau!r}, largest dropped {top!r}")
    tie = a == tau
    tk, td = np.nonzero(tie & kept)[0], np.nonzero(tie & dropped)[0]
    if len(td) and tk[-1] > td[0]:
        i = int(td[0])
        raise AssertionError(f"rule 4 (among |v| == tau = {tau!r} the lowest indices are kept) broke at index {i}: dropped, while "
                             f"index {int(tk[-1])} of the same magnitude was kept ({len(tk)} of {len(tk) + len(td)} ties kept)")


def straddles(v, k):
    """#{|v| > tau} < k < #{|v| >= tau}: the k-th place falls inside a tie group.  Returns (flag, tau, size of the group)."""
    a = np.abs(np.asarray(v))
    if not 0 < k <= len(a):
        return False, None, 0
    tau = np.sort(a)[::-1][k - 1]
    gt, ge = int((a > tau).sum()), int((a >= tau).sum())
    return bool(tau > 0 and gt < k < ge), tau, ge - gt


def warm_probes(tau_prev, TF):
    """The eight thresholds k_card_select leaves for the next search: TF(tau_prev * m), the product taken in double."""
    return [float(TF(float(tau_prev) * m)) for m in WARM]


def predict_route(v, k, TF, probes=None, cap=CAP):
    """k_card_decide's rule on the magnitudes of v (TF numbers).  probes: the eight thresholds of a warm search
    (warm_probes), None for a cold one.  Returns dict(exit = "all" | "none" | "search", passes, lo, hi, gathered): the
    refinement passes that ran, the final bracket (lo, hi] and #{lo < |v| <= hi}; `ran_out` says that the bracket still held
    more than the cap when the passes were used up; `collapsed` counts the probes of the refinement passes that the rounding
    to TF put onto an end of the bracket they were to split (such a probe decides nothing)."""
    a = np.abs(np.asarray(v).astype(TF)).astype(np.float64)
    k = int(k)
    nnz = float((a > 0).sum())
    if k >= len(a) or k >= nnz:
        return dict(exit="all", passes=0, lo=0.0, hi=0.0, gathered=0, ran_out=False)
    if k <= 0:
        return dict(exit="none", passes=0, lo=0.0, hi=0.0, gathered=0, ran_out=False)
    lo, clo, hi, chi = 0.0, nnz, float(a.max()), 0.0
    srt = np.sort(a)

    def count(t):                       # #{|v| > t}
        return float(len(srt) - np.searchsorted(srt, t, side="right"))

    def decide(ts):
        nonlocal lo, clo, hi, chi
        for t in ts:
            if not (t < np.inf) or not (t > lo) or not (t < hi):
                continue
            c = count(t)
            if c >= k:
                lo, clo = t, c
            else:
                hi, chi = t, c
        return clo - chi > cap and hi > lo

    refine = decide(list(probes) if probes is not None else [])
    passes = collapsed = 0
    while refine and passes < REFINES:
        ts = [float(TF(lo + (hi - lo) * (j + 1) / 9.0)) for j in range(8)]
        collapsed += sum(t <= lo or t >= hi for t in ts)       # probes that the rounding to TF put onto the bracket's ends
        refine = decide(ts)
        passes += 1
    return dict(exit="search", passes=passes, lo=lo, hi=hi, gathered=int(clo - chi), ran_out=bool(refine), collapsed=collapsed)


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------
def heavy(rng, n, TF):
    return (rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(TF)


LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 8191, 8192, 8193)


def length_vector(n, TF):
    """Heavy-tailed values, every seventh an exact zero and every eleventh a -0.0 (from n = 2 on: one entry stays non-zero)."""
    rng = np.random.default_rng(1000 + n)
    v = heavy(rng, n, TF)
    v[v == 0] = TF(1)
    if n > 1:
        v[1::7] = TF(0)
        v[5::11] = TF(-0.0)
    return v


def ks_for(v):
    n, nnz = len(v), int((v != 0).sum())
    return sorted({max(0, k) for k in (0, 1, 2, n // 3, nnz - 1, nnz, nnz + 1, n - 1, n, n + 5)})


def signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def named_vectors(TF):
    """[(name, v, [k, ...], class)] of the issue's table.  class: what predict_route must say about every (v, k) of the entry --
    "refined": at least one refinement pass and a final bracket within the cap; "ran-out": the bracket is still above the cap
    after the fifth pass; "collapsed": ran out, and whole passes were spent on probes that the rounding to TF put onto the ends of
    a bracket one ulp wide; "bottom": no pass, the selection runs among the smallest subnormal and normal numbers of TF.
    `cluster` in Float32 is adjacent floats, three or four entries on each, so every probe of its fourth pass is itself a tie
    value; the bracket is still 1300 ulps wide there, so none of them reaches an end: it is "refined" in both precisions.  What a
    cold search can reach of collapsed probes -- five passes narrow (0, vmax] by 9^5 < 2^16, never to an ulp of a normal number --
    is `subnormal-ties`, where an ulp is the unit: three groups of 10000 on the three smallest subnormals."""
    out = []
    rng = np.random.default_rng(4242)
    out.append(("uniform", (rng.random(100000) * signs(rng, 100000)).astype(TF), [30000], "refined"))
    v = ((1.0 + rng.random(50000)) * signs(rng, 50000)).astype(TF)
    v[31337] = TF(1e9)
    out.append(("outlier", v, [20000], "ran-out"))
    v = heavy(rng, 40000, TF)
    v[np.abs(v) == TF(0.75)] = TF(0.7)
    at = rng.choice(40000, 10000, replace=False)
    v[at] = (0.75 * signs(rng, 10000)).astype(TF)
    above = int((np.abs(v) > TF(0.75)).sum())
    out.append(("big-tie", v, [above + q for q in (1, 5000, 9999)], "ran-out"))
    out.append(("all-tie", (3.0 * signs(rng, 20000)).astype(TF), [7, 19999], "ran-out"))
    j = rng.integers(0, 8193, 30000)
    out.append(("cluster", ((1.0 + j * 2.0 ** -23) * signs(rng, 30000)).astype(TF), [10000], "refined"))
    tiny, fi = float(np.finfo(TF).tiny), np.finfo(TF)
    sub = float(np.nextafter(TF(0), TF(1)))
    mags = np.concatenate([sub * rng.integers(1, 2000, 2500), tiny * (1.0 + rng.integers(0, 2000, 2500) * float(fi.eps))])
    v = (rng.permutation(mags) * signs(rng, 5000)).astype(TF)
    out.append(("denormal", v, [1000], "bottom"))
    v = (sub * rng.integers(1, 4, 30000) * signs(rng, 30000)).astype(TF)
    two = int((np.abs(v) > TF(sub)).sum()) - int((np.abs(v) > TF(2 * sub)).sum())
    out.append(("subnormal-ties", v, [int((np.abs(v) > TF(2 * sub)).sum()) + two // 2], "collapsed"))
    return out
