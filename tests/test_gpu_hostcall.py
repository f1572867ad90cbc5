"""The five host-buffer calls (measure, lpc, iaif, filter_track, inverse_filter) in sequence on ONE engine, whose pool
buffers they share: 3 rows, then 600 rows (600 x 2048 int16 is more than the 1 MiB the buffers are grown by, so d_in and
d_aux are freed and made again), then 5 rows in the buffers the 600 left behind, with the optional arrays switched from
step to step (marks, coefs, glottal, formants, gains, ragged lengths under an out= array of sentinels).  Every result is
bit for bit what the same call gives on a fresh Engine, whose buffers nothing has used."""
import numpy as np
import pytest

import voice_synth_amd as vs
from gpu_support import same_bits

pytestmark = pytest.mark.gpu

NS, FS, K = 2048, 16000, 13
BASE = 24            # utterances synthesised; the rows of a step repeat them
TABLES = "aiu1234567"
PAST_FILL = 12345
# rows; marks; coefs and glottal; n_formants; gains; ragged lengths under sentinels
STEPS = ((3, 8, True, 5, True, False),
         (600, 0, False, 0, False, True),
         (5, 8, True, 5, True, True))


def _same(got, want):
    if isinstance(want, dict):
        assert list(got) == list(want)
        for k in want:
            same_bits(got[k], want[k])
    elif isinstance(want, tuple):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same_bits(g, w)
    else:
        same_bits(got, want)


def _calls(n, marks, sets, n_formants, with_gains, ragged, flow, pcm):
    """the five calls of one step: (name, call(engine), check(result))"""
    rows = np.arange(n) % BASE
    flow, pcm = flow[rows], pcm[rows]
    rng = np.random.default_rng(1000 + n)
    tabs = np.array([vs.vowel_coefficients(v) for v in TABLES])
    coefs = tabs[rng.integers(0, 10, (n, K))]
    gains = rng.uniform(0.5, 2.0, (n, K)) if with_gains else None
    lengths = (NS - 1 - 3 * (np.arange(n) % 50)).astype(np.int32) if ragged else None
    out = np.full((n, NS), PAST_FILL, dtype=np.int16) if ragged else None

    def measured(r):
        rec, mk = r if marks else (r, None)
        assert (rec["status"] == 0).any()
        assert mk is None or (mk.shape == (n, marks) and (mk[:, 0] >= 0).any())

    def framed(glottal):
        def check(r):
            assert (r["status"] == 0).any() and r["formants"].shape[2] == n_formants
            assert n_formants == 0 or np.isfinite(r["formants"]).any()
            assert ("coefs" in r) == sets and ("glottal" in r) == (sets and glottal)
            assert not sets or all(np.isfinite(r[k]).any() for k in ("coefs", "glottal") if k in r)
        return check

    def filtered(least):
        def check(r):
            sig, stat = r
            assert not stat["n_unusable"].any() and np.abs(sig.astype(np.int32)).max() > least
            if ragged:  # what lies past a row's length came back as it went
                past = np.arange(NS)[None, :] >= lengths[:, None]
                assert past.any() and (sig[past] == PAST_FILL).all() and (sig[~past] != PAST_FILL).any()
        return check

    return (
        ("measure", lambda e: e.measure(pcm, FS, lengths=lengths, marks=marks), measured),
        ("lpc", lambda e: e.lpc(pcm, FS, lengths=lengths, coefs=sets, n_formants=n_formants), framed(False)),
        ("iaif", lambda e: e.iaif(pcm, FS, lengths=lengths, coefs=sets, glottal=sets, n_formants=n_formants),
         framed(True)),
        ("filter_track", lambda e: e.filter_track(flow, coefs, 160, lengths=lengths, gain=2.0, pre_emphasis=0.9,
                                                  gains=gains, out=out), filtered(1000)),
        ("inverse_filter", lambda e: e.inverse_filter(pcm, coefs, 160, lengths=lengths, scale=0.5, de_emphasis=0.9,
                                                      out=out), filtered(100)),
    )


def test_host_buffer_calls_share_one_pool(engine):
    assert engine.arith == vs.VS_ARITH_EXACT
    lanes = [vs.lane_from_cli(["-r", str(FS), "-d", "1", "-j", "1", "-g", "300", "-f", "%d" % (95 + 2 * k)],
                              ["-v", TABLES[k % 10]], 500 + k)[0] for k in range(BASE)]
    flow, pcm = engine.source(lanes, NS), engine.synth(lanes, NS)
    assert np.abs(pcm.astype(np.int32)).max() > 1000
    with vs.Engine(0) as one:
        for step in STEPS:
            for name, call, check in _calls(*step, flow, pcm):
                got = call(one)
                check(got)
                with vs.Engine(0) as fresh:
                    _same(got, call(fresh))
