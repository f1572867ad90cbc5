"""The set walk that csrc/vs_track.hip and csrc/vs_inverse.hip each have a copy of, held directly: the round trip between
the two kernels rests on the copies being equal, which each kernel's own byte-for-byte test cannot see.  The same sets
and the same (n_sets, hop, offset, length) go through vs_track_launch and vs_inverse_launch, and

  - status and n_unusable of the two kernels agree row by row, with each other, with track_ref.usable and with the
    restatements' stat;
  - the inverse of the track's output (scale = 1 / gain, de_emphasis = pre_emphasis) stays within the bound of
    include/voice_synth.h, "inverse filtering", consequence (c), on every row that has a set -- which it can only do when
    both kernels ran the same taps at the same sample.

96 rows (a whole wavefront and half of one) x 600 samples, hold and glide, orders 22 and 40, exact arithmetic, no per-set
gains (tests/test_gpu_track_hostile.py has those).  The rows make the walk diverge inside a wavefront: hops 24, 25, 160
and 1 and offsets -50, 0, 7 and beyond the row's end mixed across lanes, 1 to 30 sets per row, so some rows never reach
their last sets.  A NaN tap sits in the first set, a middle one, the last one reached, one never reached, in several of
these, and in a few rows in every set; in glide mode some sets are finite with one |k_i| >= 1, which hold would accept.

The bound.  The header derives it for a constant set; for these rows the same derivation gives a bound per sample.  The
track wrote x = y[n] - mu*y[n-1] + r[n] with |r[n]| <= 0.5 (no sample clipped: asserted), y the all-pole output on
g*flow.  The inverse is linear: its de-emphasis returns u = y + w, w = r / (1 - mu z^-1), and its FIR with the taps of
sample n returns sum_j a_j(n) y[n-j] + sum_j a_j(n) w[n-j].  The first sum is g*flow[n] because the track ran the SAME
a_j(n) at sample n; the second is sum_i h_n[i] r[n-i] with h_n the impulse response of A_n(z) / (1 - mu z^-1), A_n the
taps in force at sample n whatever ran before.  So |inverse - flow|[n] <= 0.5*scale*sum|h_n| + 1.5 =
inverse_ref.round_trip_bound(A_n, ...), and a row's bound is the largest over the groups of 24 samples it has, with the
taps the restatement's walk gives for each group (track_ref.filter_track(taps=...)): interpolated sets included.

The first test runs without a GPU: the restatements alone satisfy every assertion on these inputs, and the inputs are
what the text above says they are."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import voice_synth_amd as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_ref as ir  # noqa: E402
import track_ref as tr  # noqa: E402

R, N, S = 96, 600, 30
HOPS = (24, 25, 160, 1)
OFFSETS = (-50, 0, 7, N + 100)
EVERY = (9, 40, 71, 95)                          # rows with a NaN in every set
SHORT = {13: 577, 29: 25, 45: 24, 61: 1, 77: 0, 93: 313}
MODE_NAME = {tr.HOLD: "hold", tr.GLIDE: "glide"}
CASES = [(mode, order) for mode in (tr.HOLD, tr.GLIDE) for order in (22, 40)]


def _walk(K, hop, offset, length):
    """[rows][groups]: the k of every group of 24 samples (-1 behind the row's length)"""
    m = np.arange(0, N, tr.GROUP)[None, :]
    mo = m - offset[:, None]
    k = np.where(mo < 0, 0, np.minimum(mo // hop[:, None], K[:, None] - 1))
    return np.where(m < length[:, None], k, -1)


@functools.lru_cache(maxsize=None)
def case(mode, order):
    rng = np.random.default_rng(20250 + 100 * mode + order)
    r = np.arange(R)
    K = 1 + (7 * r) % S
    hop = np.array(HOPS)[r % 4]
    offset = np.array(OFFSETS)[(r // 4) % 4]
    length = np.full(R, N)
    for row, n in SHORT.items():
        length[row] = n
    gain = np.array([1.0, 0.5, 2.0])[r % 3]
    mu = np.array([0.0, 0.5, 0.9, 0.97], dtype=np.float32)[(r // 2) % 4]
    k = _walk(K, hop, offset, length)
    last = np.maximum(k.max(axis=1), 0)          # the last set the walk reaches

    # stable sets: convex blends of the tables in the reflection domain, small further coefficients beyond 22 taps
    kt = np.array([tr.reflection(vs.vowel_coefficients(v))[0] for v in "aiu1234567"])
    w = rng.uniform(0, 1, (R, S, 1))
    kap = w * kt[rng.integers(0, 10, (R, S))] + (1.0 - w) * kt[rng.integers(0, 10, (R, S))]
    if order > 22:
        kap = np.concatenate([kap, rng.uniform(-0.2, 0.2, (R, S, order - 22))], axis=2)
    kap = kap[..., :order]
    big = np.zeros((R, S), dtype=bool)           # glide: finite sets with one |k_i| >= 1
    if mode == tr.GLIDE:
        for row in r[r % 3 == 1]:
            s = (5 * row) % K[row]
            kap[row, s, (3 * row) % order] = 1.25 if row % 2 else -1.25
            big[row, s] = True
    coefs = tr.step_up(kap)
    assert np.isfinite(coefs).all()

    nan = np.zeros((R, S), dtype=bool)
    kind = r // 16                               # 0 none, 1 first, 2 middle, 3 last reached, 4 unreached, 5 all of these
    for row in r:
        at = {0: [], 1: [0], 2: [last[row] // 2 if last[row] >= 2 else K[row] // 2], 3: [last[row]], 4: [K[row] - 1],
              5: [0, last[row] // 2, last[row], K[row] - 1]}[kind[row]]
        if row in EVERY:
            at = range(K[row])
        for s in at:
            nan[row, min(s, K[row] - 1)] = True
            coefs[row, min(s, K[row] - 1), 1 + row % order] = np.nan

    flow = rng.integers(-100, 101, (R, N)).astype(np.int16)
    trows = vs.track_rows(R, K, hop, offset, length, gain, mu)
    irows = vs.inverse_rows(R, K, hop, offset, length, 1.0 / gain, mu)

    # what the header's step 1 says of these sets
    ok, _ = tr.usable(coefs, mode)
    inK = np.arange(S)[None, :] < K[:, None]
    n_unusable = (inK & ~ok).sum(axis=1)
    none = ~(ok & inK).any(axis=1)

    # the restatements, and the bound of every row from the taps of its groups
    taps = []
    pcm, tstat = tr.filter_track(flow, coefs, trows, mode, taps=taps)
    res, istat = ir.inverse_filter(pcm, coefs, irows, mode)
    bound = np.zeros(R)
    for g, a in enumerate(taps):
        for row in r[(k[:, g] >= 0) & ~none]:
            A = np.concatenate([[1.0], a[row]])
            bound[row] = max(bound[row], ir.round_trip_bound(A, mu[row], irows["scale"][row], int(length[row])))
    for a in (flow, coefs, pcm, res, bound):
        a.setflags(write=False)
    return SimpleNamespace(mode=mode, order=order, K=K, hop=hop, offset=offset, length=length, k=k, last=last, nan=nan,
                           big=big, inK=inK, flow=flow, coefs=coefs, trows=trows, irows=irows, n_unusable=n_unusable,
                           none=none, pcm=pcm, tstat=tstat, res=res, istat=istat, bound=bound)


def _check(c, pcm, tstat, res, istat, what):
    """the assertions of this file on (track output, track stat, inverse output, inverse stat) of case c"""
    assert np.array_equal(tstat["status"], istat["status"]), what
    assert np.array_equal(tstat["n_unusable"], istat["n_unusable"]), what
    assert np.array_equal(tstat["n_unusable"], c.n_unusable), (what, tstat["n_unusable"], c.n_unusable)
    assert np.array_equal(tstat["status"], np.where(c.none, tr.NO_SET, 0)), what
    inside = np.arange(N)[None, :] < c.length[:, None]
    live = inside & ~c.none[:, None]
    assert np.abs(pcm.astype(np.int32))[live].max() < 32767 and not istat["n_clipped"].any(), what
    assert not pcm[inside & c.none[:, None]].any() and not res[inside & c.none[:, None]].any(), what
    err = np.where(live, np.abs(res.astype(np.int32) - c.flow.astype(np.int32)), 0).max(axis=1)
    print("%s, %s order %d: %d rows with a set, largest |inverse - flow| %d LSB (bound there %.1f), smallest margin %.1f LSB; "
          "n_unusable %d in all, %d rows without a set" % (what, MODE_NAME[c.mode], c.order, int((~c.none).sum()),
                                                          err.max(), c.bound[np.argmax(err)],
                                                          (c.bound - err)[~c.none & (c.length > 0)].min(), int(c.n_unusable.sum()),
                                                          int(c.none.sum())))
    assert (err <= c.bound)[~c.none].all(), (what, np.flatnonzero(err > c.bound), err, c.bound)
    return err


@pytest.mark.parametrize("mode,order", CASES)
def test_the_restatements_alone_hold_every_assertion(mode, order):
    c = case(mode, order)
    err = _check(c, c.pcm, c.tstat, c.res, c.istat, "restatements")
    assert err.max() >= 1                        # (the round trip is not an identity: something is measured)
    # the inputs are what the module's text says
    for wave in (slice(0, 64), slice(64, R)):
        kw = c.k[wave]
        assert max(len(set(col[col >= 0])) for col in kw.T) >= 4            # lanes of one wavefront on different sets
        moves = (np.diff(kw, axis=1) != 0) & (kw[:, 1:] >= 0)
        assert (moves.any(axis=0) & ~moves.all(axis=0)).any()               # some lanes advance where others do not
    assert (c.last < c.K - 1).sum() >= 10 and (c.last == c.K - 1).sum() >= 10   # rows that do not reach their last sets
    assert (c.offset > c.length).any() and sorted(set(c.K)) == list(range(1, S + 1))
    rows = np.arange(R)
    assert (c.nan[:, 0] & ~c.none).any()                                     # the first set, the row still has one
    assert (c.nan[rows, c.last] & (c.last > 0) & ~c.none).any()              # the last set reached
    assert ((c.nan & c.inK & (np.arange(S)[None, :] > c.last[:, None])).any(axis=1) & ~c.none).any()   # one never reached
    mid = (np.arange(S)[None, :] > 0) & (np.arange(S)[None, :] < c.last[:, None])
    assert ((c.nan & mid).any(axis=1) & ~c.none).any()                       # a middle one
    assert all(c.none[row] and c.n_unusable[row] == c.K[row] for row in EVERY)
    assert 4 <= c.none.sum() <= 12
    if mode == tr.GLIDE:                         # hold accepts what glide refuses
        only = c.big & ~c.nan
        assert only.sum() >= 20 and tr.usable(c.coefs, tr.HOLD)[0][only].all() and not tr.usable(c.coefs, tr.GLIDE)[0][only].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,order", CASES)
def test_track_and_inverse_walk_the_same_sets(engine, mode, order):
    c = case(mode, order)
    name = MODE_NAME[mode]
    with engine.scope() as dev:
        bufs = [dev.room(R * N * 2) for _ in range(3)]
        flow_d, pcm_d, res_d = bufs
        bufs += [dev.room(c.coefs.nbytes), dev.room(R * 8), dev.room(R * 16)]
        cf_d, tst_d, ist_d = bufs[3:]
        engine.dev_upload(flow_d, c.flow)
        engine.dev_upload(cf_d, c.coefs)
        for p in (pcm_d, res_d):
            engine.dev_upload(p, np.zeros((R, N), dtype=np.int16))
        # the inverse right behind the track filter on the stream, on the track's output
        engine.filter_track_dev(name, order, flow_d, N, pcm_d, N, R, N, c.trows, cf_d, S, stat_ptr=tst_d)
        engine.inverse_filter_dev(name, order, pcm_d, N, res_d, N, R, N, c.irows, cf_d, S, stat_ptr=ist_d)
        pcm = engine.dev_download(pcm_d, (R, N))
        res = engine.dev_download(res_d, (R, N))
        tstat = engine.dev_download(tst_d, (R,), vs.TRACK_STAT_DTYPE)
        istat = engine.dev_download(ist_d, (R,), vs.INVERSE_STAT_DTYPE)
    _check(c, pcm, tstat, res, istat, "device")
    # and with the restatements, byte for byte
    assert np.array_equal(tstat, c.tstat.astype(vs.TRACK_STAT_DTYPE)) and np.array_equal(pcm, c.pcm)
    assert np.array_equal(istat, c.istat.astype(vs.INVERSE_STAT_DTYPE)) and np.array_equal(res, c.res)
