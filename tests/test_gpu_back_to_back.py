"""Two device-pointer launches of one entry point back to back (measure_dev, lpc_dev, filter_track_dev,
inverse_filter_dev, iaif_dev): the second is enqueued while the first one's record upload may still be on its way out of
the context's pinned block.  Call A has 3 rows; call B, with no wait in between, has 70 rows (two 64-lane workgroups)
with other per-row values, so it grows the pinned block and takes another device block.  Both write into buffers of their
own on the same stream; after one wait both are bit for bit what the host-buffer calls (measure, lpc, filter_track,
inverse_filter, iaif; VS_ARITH_EXACT) give for the same inputs."""
import numpy as np
import pytest

import voice_synth_amd as vs
from gpu_support import same_bits

pytestmark = pytest.mark.gpu

NS, FS = 2048, 16000
NA, NB = 3, 70
TABLES = "aiu1234567"
# what call B says of its rows (call A: FS and NS for all): other rates, so other lag bounds and window lengths
FS_B = np.array([16000, 12000, 22050, 8000, 11025], dtype=np.int32)[np.arange(NB) % 5]
LEN_B = (NS - 7 * np.arange(NB)).astype(np.int32)

_rows = {}


def _signals(engine):
    """NA + NB utterances of NS samples at FS, synthesised once: (flow, pcm)"""
    if not _rows:
        lanes = [vs.lane_from_cli(["-r", str(FS), "-d", "1", "-j", "1", "-g", "300", "-f", "%d" % (95 + 2 * k)],
                                  ["-v", TABLES[k % 10]], 300 + k)[0] for k in range(NA + NB)]
        _rows["flow"], _rows["pcm"] = engine.source(lanes, NS), engine.synth(lanes, NS)
        assert np.abs(_rows["pcm"].astype(np.int32)).max() > 1000
    return _rows["flow"], _rows["pcm"]


def _measure(engine):
    _, pcm = _signals(engine)
    with engine.scope() as dev:
        pcm_d = dev.put(pcm)
        out_a, out_b = dev.put(np.zeros(NA, dtype=vs.ACOUSTIC_DTYPE)), dev.put(np.zeros(NB, dtype=vs.ACOUSTIC_DTYPE))
        engine.measure_dev(pcm_d, NS, NA, NS, FS, out_a)
        engine.measure_dev(pcm_d + NA * NS * 2, NS, NB, NS, FS_B, out_b, lengths=LEN_B)
        engine.synchronize()
        got_a = dev.get(out_a, (NA,), vs.ACOUSTIC_DTYPE)
        got_b = dev.get(out_b, (NB,), vs.ACOUSTIC_DTYPE)
    assert (got_a["status"] == 0).any() and (got_b["status"] == 0).any()
    same_bits(got_a, engine.measure(pcm[:NA], FS))
    same_bits(got_b, engine.measure(pcm[NA:], FS_B, lengths=LEN_B))


def _lpc_fill(n, fp):
    """what Engine.lpc hands in: frames no row reaches keep it"""
    fr = np.zeros((n, fp), dtype=vs.LPC_FRAME_DTYPE)
    fr["r0"] = fr["err"] = np.nan
    fr["start"] = fr["status"] = -1
    return fr, np.full((n, fp, 5, 2), np.nan), np.full((n, fp, 23), np.nan)


def _lpc(engine):
    _, pcm = _signals(engine)
    fp_a = vs.lpc_frames(FS, NS)
    fp_b = max(vs.lpc_frames(int(f), int(l)) for f, l in zip(FS_B, LEN_B))
    assert fp_a >= 3 and len(set(np.floor(0.025 * FS_B + 0.5))) == 5
    with engine.scope() as dev:
        pcm_d = dev.put(pcm)
        a = [dev.put(x) for x in _lpc_fill(NA, fp_a)]
        b = [dev.put(x) for x in _lpc_fill(NB, fp_b)]
        engine.lpc_dev(pcm_d, NS, NA, NS, FS, fp_a, *a)
        engine.lpc_dev(pcm_d + NA * NS * 2, NS, NB, NS, FS_B, fp_b, *b, lengths=LEN_B)
        engine.synchronize()
        got = []
        for n, fp, ptrs in ((NA, fp_a, a), (NB, fp_b, b)):
            got.append((dev.get(ptrs[0], (n, fp), vs.LPC_FRAME_DTYPE),
                        dev.get(ptrs[1], (n, fp, 5, 2), np.float64),
                        dev.get(ptrs[2], (n, fp, 23), np.float64)))
    for (fr, fm, cf), want in ((got[0], engine.lpc(pcm[:NA], FS, coefs=True)),
                               (got[1], engine.lpc(pcm[NA:], FS_B, lengths=LEN_B, coefs=True))):
        assert (want["status"] == 0).any()
        for k in ("r0", "err", "start", "status", "n_formants"):
            same_bits(fr[k], want[k])
        same_bits(fm, want["formants"])
        same_bits(cf, want["coefs"])


def _track(engine):
    flow, _ = _signals(engine)
    K = 13
    rng = np.random.default_rng(20241017)
    tabs = np.array([vs.vowel_coefficients(v) for v in TABLES])
    coefs = tabs[rng.integers(0, 10, (NA + NB, K))]
    rows_a = vs.track_rows(NA, K, 160, 0, NS, 2.0, 1.0)
    rows_b = vs.track_rows(NB, 1 + np.arange(NB) % K, 100 + np.arange(NB), 3 * np.arange(NB) - 50, LEN_B, 1.5, 0.9)
    with engine.scope() as dev:
        flow_d, cf_d = dev.put(flow), dev.put(coefs)
        out_a, out_b = dev.put(np.zeros((NA, NS), dtype=np.int16)), dev.put(np.zeros((NB, NS), dtype=np.int16))
        st_a, st_b = dev.put(np.zeros(NA, dtype=vs.TRACK_STAT_DTYPE)), dev.put(np.zeros(NB, dtype=vs.TRACK_STAT_DTYPE))
        engine.filter_track_dev("hold", 22, flow_d, NS, out_a, NS, NA, NS, rows_a, cf_d, K, stat_ptr=st_a)
        engine.filter_track_dev("hold", 22, flow_d + NA * NS * 2, NS, out_b, NS, NB, NS, rows_b, cf_d + NA * K * 23 * 8,
                                K, stat_ptr=st_b)
        engine.synchronize()
        got_a = dev.get(out_a, (NA, NS)), dev.get(st_a, (NA,), vs.TRACK_STAT_DTYPE)
        got_b = dev.get(out_b, (NB, NS)), dev.get(st_b, (NB,), vs.TRACK_STAT_DTYPE)
    want_a = engine.filter_track(flow[:NA], coefs[:NA], 160, gain=2.0, pre_emphasis=1.0)
    want_b = engine.filter_track(flow[NA:], coefs[NA:], rows_b["hop"], rows_b["offset"], rows_b["n_sets"], LEN_B, 1.5, 0.9)
    for got, want in ((got_a, want_a), (got_b, want_b)):
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        assert not want[1]["status"].any() and np.abs(want[0].astype(np.int32)).max() > 1000


def _inverse(engine):
    _, pcm = _signals(engine)
    K = 13
    rng = np.random.default_rng(20241019)
    tabs = np.array([vs.vowel_coefficients(v) for v in TABLES])
    coefs = tabs[rng.integers(0, 10, (NA + NB, K))]
    rows_a = vs.inverse_rows(NA, K, 160, 0, NS, 0.5, 1.0)
    rows_b = vs.inverse_rows(NB, 1 + np.arange(NB) % K, 100 + np.arange(NB), 3 * np.arange(NB) - 50, LEN_B, 0.25, 0.9)
    with engine.scope() as dev:
        pcm_d, cf_d = dev.put(pcm), dev.put(coefs)
        out_a, out_b = dev.put(np.zeros((NA, NS), dtype=np.int16)), dev.put(np.zeros((NB, NS), dtype=np.int16))
        st_a = dev.put(np.zeros(NA, dtype=vs.INVERSE_STAT_DTYPE))
        st_b = dev.put(np.zeros(NB, dtype=vs.INVERSE_STAT_DTYPE))
        engine.inverse_filter_dev("hold", 22, pcm_d, NS, out_a, NS, NA, NS, rows_a, cf_d, K, stat_ptr=st_a)
        engine.inverse_filter_dev("hold", 22, pcm_d + NA * NS * 2, NS, out_b, NS, NB, NS, rows_b, cf_d + NA * K * 23 * 8,
                                  K, stat_ptr=st_b)
        engine.synchronize()
        got_a = dev.get(out_a, (NA, NS)), dev.get(st_a, (NA,), vs.INVERSE_STAT_DTYPE)
        got_b = dev.get(out_b, (NB, NS)), dev.get(st_b, (NB,), vs.INVERSE_STAT_DTYPE)
    want_a = engine.inverse_filter(pcm[:NA], coefs[:NA], 160, scale=0.5, de_emphasis=1.0)
    want_b = engine.inverse_filter(pcm[NA:], coefs[NA:], rows_b["hop"], rows_b["offset"], rows_b["n_sets"], LEN_B, 0.25, 0.9)
    for got, want in ((got_a, want_a), (got_b, want_b)):
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        assert not want[1]["n_unusable"].any() and np.abs(want[0].astype(np.int32)).max() > 100


def _iaif_fill(n, fp):
    """what Engine.iaif hands in: _lpc_fill and the glottal sets"""
    return _lpc_fill(n, fp) + (np.full((n, fp, 5), np.nan),)


def _iaif(engine):
    _, pcm = _signals(engine)
    fp_a = vs.lpc_frames(FS, NS, **vs.iaif_lpc_opts())
    fp_b = max(vs.lpc_frames(int(f), int(l), **vs.iaif_lpc_opts()) for f, l in zip(FS_B, LEN_B))
    assert fp_a >= 3
    with engine.scope() as dev:
        pcm_d = dev.put(pcm)
        a = [dev.put(x) for x in _iaif_fill(NA, fp_a)]
        b = [dev.put(x) for x in _iaif_fill(NB, fp_b)]
        engine.iaif_dev(pcm_d, NS, NA, NS, FS, fp_a, *a)
        engine.iaif_dev(pcm_d + NA * NS * 2, NS, NB, NS, FS_B, fp_b, *b, lengths=LEN_B)
        engine.synchronize()
        got = []
        for n, fp, ptrs in ((NA, fp_a, a), (NB, fp_b, b)):
            got.append((dev.get(ptrs[0], (n, fp), vs.LPC_FRAME_DTYPE),
                        dev.get(ptrs[1], (n, fp, 5, 2), np.float64),
                        dev.get(ptrs[2], (n, fp, 23), np.float64),
                        dev.get(ptrs[3], (n, fp, 5), np.float64)))
    for (fr, fm, cf, gl), want in ((got[0], engine.iaif(pcm[:NA], FS, coefs=True, glottal=True)),
                                   (got[1], engine.iaif(pcm[NA:], FS_B, lengths=LEN_B, coefs=True, glottal=True))):
        assert (want["status"] == 0).any()
        for k in ("r0", "err", "start", "status", "n_formants"):
            same_bits(fr[k], want[k])
        same_bits(fm, want["formants"])
        same_bits(cf, want["coefs"])
        same_bits(gl, want["glottal"])


ENTRIES = {"measure_dev": _measure, "lpc_dev": _lpc, "filter_track_dev": _track, "inverse_filter_dev": _inverse,
           "iaif_dev": _iaif}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_second_launch_before_the_first_upload_is_waited_for(engine, entry):
    assert engine.arith == vs.VS_ARITH_EXACT
    ENTRIES[entry](engine)
