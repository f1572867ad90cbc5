"""The helpers of the GPU tests, held on the CPU: Engine.scope() (voice_synth_amd.DeviceScope) on an engine that is a dict of
bytearrays, and the numpy half of tests/gpu_support.py."""
import itertools

import numpy as np
import pytest

import voice_synth_amd as vs
import gpu_support as gs


class FakePlan:
    def __init__(self, engine):
        self.engine = engine
        engine.open_plans.append(self)

    def close(self):
        self.engine.events.append(("close", self))
        self.engine.open_plans.remove(self)


class FakeEngine:
    """device memory as a dict of bytearrays; events: every free and close in the order it happened"""

    def __init__(self, failing_frees=()):
        self.mem, self.events, self.open_plans, self.next = {}, [], [], 0x1000
        self.failing_frees = set(failing_frees)

    def dev_alloc(self, nbytes):
        assert nbytes >= 1
        ptr, self.next = self.next, self.next + ((nbytes + 255) & ~255)
        self.mem[ptr] = bytearray(nbytes)
        return ptr

    def dev_free(self, ptr):
        self.events.append(("free", ptr))
        del self.mem[ptr]                        # a second free of the same pointer is a KeyError
        if ptr in self.failing_frees:
            raise vs.VsError(-1, "vs_dev_free")

    def dev_upload(self, ptr, array):
        raw = np.ascontiguousarray(array).tobytes()
        self.mem[ptr][:len(raw)] = raw

    def dev_download(self, ptr, shape, dtype=np.int16):
        out = np.empty(shape, dtype=dtype)
        return np.frombuffer(bytes(self.mem[ptr][:out.nbytes]), dtype=dtype).reshape(shape).copy()

    def plan(self, lanes, n_samples):
        return FakePlan(self)

    scope = vs.Engine.scope


def _fill(dev):
    """three buffers and two plans, interleaved; returns (pointers, plans) in creation order"""
    a = dev.room(0)
    p = dev.plan([], 10)
    b = dev.put(np.arange(5, dtype=np.int32))
    q = dev.plan([], 10)
    c = dev.filled(3, 0x5A5A, np.int16)
    return [a, b, c], [p, q]


def _released_once_in_reverse(eng, ptrs, plans):
    assert eng.events == [("close", q) for q in reversed(plans)] + [("free", p) for p in reversed(ptrs)]
    assert not eng.mem and not eng.open_plans


def test_scope_hands_out_what_it_says():
    eng = FakeEngine()
    with eng.scope() as dev:
        ptrs, _ = _fill(dev)
        assert len(eng.mem[ptrs[0]]) == 1
        assert np.array_equal(dev.get(ptrs[1], (5,), np.int32), np.arange(5))
        assert np.array_equal(dev.get(ptrs[2], (3,)), np.full(3, 0x5A5A, dtype=np.int16))
        assert not eng.events


def test_scope_frees_everything_once_in_reverse_on_a_clean_exit():
    eng = FakeEngine()
    with eng.scope() as dev:
        ptrs, plans = _fill(dev)
    _released_once_in_reverse(eng, ptrs, plans)


def test_scope_frees_everything_once_in_reverse_when_the_body_raises():
    eng = FakeEngine()
    with pytest.raises(ZeroDivisionError):
        with eng.scope() as dev:
            ptrs, plans = _fill(dev)
            1 / 0
    _released_once_in_reverse(eng, ptrs, plans)


def test_the_bodys_exception_surfaces_when_a_free_raises_too():
    eng = FakeEngine()
    with pytest.raises(AssertionError, match="the real failure"):
        with eng.scope() as dev:
            ptrs, plans = _fill(dev)
            eng.failing_frees.add(ptrs[1])
            raise AssertionError("the real failure")
    _released_once_in_reverse(eng, ptrs, plans)


def test_a_failing_free_propagates_from_a_clean_exit_after_the_rest_is_released():
    eng = FakeEngine()
    with pytest.raises(vs.VsError):
        with eng.scope() as dev:
            ptrs, plans = _fill(dev)
            eng.failing_frees.add(ptrs[2])
    _released_once_in_reverse(eng, ptrs, plans)


def test_engine_plan_and_node_close_on_exit():
    for cls in (vs.Engine, vs.Plan, vs.Node):
        obj = cls.__new__(cls)
        closed = []
        obj.close = lambda: closed.append(1)
        with pytest.raises(ZeroDivisionError):
            with obj as entered:
                assert entered is obj
                1 / 0
        assert closed == [1]
        obj.close = lambda: None                 # (for __del__)


# ---- GuardedRows.check

ROWS, N = 3, 5
LAYOUTS = list(itertools.product((5, 6, 11), (0, 2)))        # (pitch, offset in bytes)


def _room(pitch, offset_bytes):
    """(the description for the largest layout, a clean room with a body drawn into it, the body, where it starts)"""
    g = gs.GuardedRows(ROWS, N, 11, 2)
    assert g.room == ROWS * 11 + 2 * gs.GUARD + 1 + 1
    whole = g.clean()
    body = np.arange(1, ROWS * N + 1, dtype=np.int16).reshape(ROWS, N)
    lead = gs.GUARD + offset_bytes // 2
    whole[lead:lead + ROWS * pitch].reshape(ROWS, pitch)[:, :N] = body
    return g, whole, body, lead


@pytest.mark.parametrize("pitch,offset_bytes", LAYOUTS)
def test_a_clean_buffer_returns_exactly_the_body(pitch, offset_bytes):
    g, whole, body, _ = _room(pitch, offset_bytes)
    got = g.check(whole, pitch, offset_bytes, "clean")
    assert got.shape == (ROWS, N) and np.array_equal(got, body)


PLACES = ["first lead", "last lead", "first tail", "last of the room", "first padding of row 0", "last padding of the last row"]


@pytest.mark.parametrize("pitch,offset_bytes,place", [(p, o, place) for p, o in LAYOUTS for place in PLACES
                                                      if p > N or "padding" not in place])
def test_one_dirty_sample_outside_the_body_is_caught(pitch, offset_bytes, place):
    g, whole, _, lead = _room(pitch, offset_bytes)
    end = lead + ROWS * pitch
    at = {"first lead": 0, "last lead": lead - 1, "first tail": end, "last of the room": g.room - 1,
          "first padding of row 0": lead + N, "last padding of the last row": end - 1}[place]
    assert whole[at] == gs.SENTINEL
    whole[at] ^= 1
    with pytest.raises(AssertionError, match="dirty"):
        g.check(whole, pitch, offset_bytes, "dirty " + place)


@pytest.mark.parametrize("pitch,offset_bytes", LAYOUTS)
def test_a_changed_sample_inside_the_body_is_not_the_guards_business(pitch, offset_bytes):
    g, whole, body, lead = _room(pitch, offset_bytes)
    for r, k in ((0, 0), (1, 2), (ROWS - 1, N - 1)):
        whole[lead + r * pitch + k] = gs.SENTINEL
        body[r, k] = gs.SENTINEL
    assert np.array_equal(g.check(whole, pitch, offset_bytes, "body"), body)


def test_the_device_half_on_the_fake_engine():
    eng = FakeEngine()
    with eng.scope() as dev:
        g = gs.GuardedRows(ROWS, N, 11, 2).on(dev)
        assert g.first(11, 2) == g.ptr + 2 * gs.GUARD + 2
        for pitch, off in LAYOUTS:
            _, whole, body, _ = _room(pitch, off)
            eng.dev_upload(g.ptr, whole)
            assert np.array_equal(g.rows_back(pitch, off, (pitch, off)), body)
            whole[-1] = 0
            eng.dev_upload(g.ptr, whole)
            with pytest.raises(AssertionError):
                g.rows_back(pitch, off, (pitch, off))
            g.fill()
            assert (dev.get(g.ptr, (g.room,)) == gs.SENTINEL).all()
        with pytest.raises(AssertionError):
            g.first(12, 2)                       # a layout the room was not sized for
    assert not eng.mem


# ---- staged_input, same_bits, same_rows

@pytest.mark.parametrize("pitch,offset", [(5, 0), (6, 0), (11, 1), (5, 1)])
def test_staged_input_puts_the_rows_behind_guard_and_offset(pitch, offset):
    rows = np.arange(1, ROWS * N + 1, dtype=np.int16).reshape(ROWS, N)
    staged = gs.staged_input(rows, pitch, offset=offset)
    lead = gs.GUARD + offset
    assert staged.dtype == np.int16 and staged.ndim == 1 and len(staged) >= lead + ROWS * pitch + gs.GUARD
    body = staged[lead:lead + ROWS * pitch].reshape(ROWS, pitch)
    assert np.array_equal(body[:, :N], rows)
    assert (body[:, N:] == gs.INPUT_PAD).all()
    assert (staged[:lead] == gs.INPUT_PAD).all() and (staged[lead + ROWS * pitch:] == gs.INPUT_PAD).all()
    other = gs.staged_input(rows, pitch, pad=0x1111, guard=2, offset=offset)
    assert (other[:2 + offset] == 0x1111).all() and np.array_equal(other[2 + offset:2 + offset + N], rows[0])


def test_same_bits_and_same_rows():
    a = np.array([0.0, 1.0])
    gs.same_bits(a, a.copy())
    gs.same_rows(a, a.copy(), "equal")
    for other in (np.array([-0.0, 1.0]), a.astype(np.float32), a[:1]):
        with pytest.raises(AssertionError):
            gs.same_bits(a, other)
    with pytest.raises(AssertionError, match="what it was"):
        gs.same_rows(np.zeros((2, 3)), np.eye(2, 3), "what it was")
    with pytest.raises(AssertionError):
        gs.same_rows(np.zeros((2, 3)), np.zeros((2, 4)), "shape")
