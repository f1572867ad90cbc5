"""The ten A(z) tables: product copy == oracle copy == numbers in the reference source text
(the last check against digests of the source text's numbers, tests/golden/reference_runs.json.gz)."""
import ctypes as C

import numpy as np

import voice_synth_amd as vs
from oracle import pyoracle as po

IDS = "aiu1234567"


def _oracle_table(v):
    lane = vs.default_lane()
    lane.vowel = ord(v)
    a = (C.c_double * 23)()
    assert po.load().vs_oracle_coefficients(C.byref(lane), a) == 0
    return np.array(a[:])


def test_product_equals_oracle():
    for v in IDS:
        assert np.array_equal(vs.vowel_coefficients(v), _oracle_table(v)), v


def test_all_tables_monic_and_stable():
    for v in IDS:
        a = vs.vowel_coefficients(v)
        assert a[0] == 1.0 and len(a) == 23
        radius = np.abs(np.roots(a)).max()
        assert radius < 1.0, (v, radius)  # 0.9747 .. 0.9921


def test_unknown_vowel_rejected():
    a = (C.c_double * 23)()
    for v in "eoxAIU089":
        assert vs.load().vs_vowel_coefficients(ord(v), a) == vs._ffi.VS_ERR_RANGE


def test_tables_match_reference_text():
    """vowel_new.c's arrays A_a ... A_zz7, parsed as doubles by oracle/gen_reference_runs.py: their count and a sha256
    of their float64 bytes"""
    ref = po.reference_tables()
    names = {"a": "A_a", "i": "A_i", "u": "A_u"}
    names.update({str(k): "A_zz%d" % k for k in range(1, 8)})
    assert sorted(ref) == sorted(names.values())
    for v, n in names.items():
        ours = np.ascontiguousarray(vs.vowel_coefficients(v), dtype="<f8")
        assert ours.size == ref[n]["n"] and po.digest(ours.tobytes()) == ref[n]["sha256"], v
