"""What the GPU tests share: the sentinel constants, the bit-for-bit comparisons, the context that takes a wave-specialised
kernel, and the guarded output (rows inside sentinel-filled device memory whose guards and pitch padding must come back
untouched).  A plain module, imported like track_ref; device memory comes from an Engine.scope() of the caller's."""
import numpy as np

import voice_synth_amd as vs

SENTINEL = 0x5A5A            # what memory a launch must not write holds
GUARD = 8                    # samples of sentinel kept in front of and behind the output rows
INPUT_PAD = 0x7777           # what the padding of a staged input holds: not silence


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes()


def same_rows(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8])


def ws_engine(arith, roles, pairs, ready):
    """a context whose plans take the wave-specialised kernel in that shape.  ready: the two-role kernel's filter
    wavefront waits for all of its lanes (64: they share one position) or runs with half of them (32: each lane has its
    own position); the three-role kernel always waits for all.  Where several groups share a workgroup the rings are
    as short as the plan allows (it lifts the 240 slots asked for to what the batch's longest period needs), so that
    four of them fit the LDS: the plan would quietly take fewer groups otherwise."""
    eng = vs.Engine(0, arith=arith)
    kw = dict(kernel=vs.VS_KERNEL_WS, ws_roles=roles, ws_pairs=pairs)
    if ready:
        kw["ready_min"] = ready
    if pairs > 1:
        kw["ring_slots"] = 240
    eng.set_tuning(**kw)
    return eng


class GuardedRows:
    """an output allocation for rows x n items at any pitch up to max_pitch and any base up to max_offset_bytes past the
    front guard: rows * max_pitch + 2 * GUARD + 1 items and the offset, all of them the sentinel before a launch.
    check() is numpy alone; on(), fill(), first() and rows_back() are the same on a DeviceScope."""

    def __init__(self, rows, n, max_pitch, max_offset_bytes=0, sentinel=SENTINEL, dtype=np.int16):
        self.rows, self.n, self.sentinel, self.dtype = rows, n, sentinel, np.dtype(dtype)
        self.room = rows * max_pitch + 2 * GUARD + 1 + -(-max_offset_bytes // self.dtype.itemsize)
        self.dev = self.ptr = None

    def clean(self):
        return np.full(self.room, self.sentinel, dtype=self.dtype)

    def on(self, dev):
        """the room, sentinel-filled, in the scope's device memory"""
        self.dev, self.ptr = dev, dev.put(self.clean())
        return self

    def fill(self):
        """the sentinel everywhere again (before the next launch of a loop over layouts)"""
        self.dev.engine.dev_upload(self.ptr, self.clean())

    def first(self, pitch, offset_bytes=0):
        """the pointer a launch at that pitch and base offset gets: behind the front guard, the back guard inside the room"""
        assert offset_bytes + (self.rows * pitch + 2 * GUARD) * self.dtype.itemsize <= self.room * self.dtype.itemsize
        return self.ptr + GUARD * self.dtype.itemsize + offset_bytes

    def rows_back(self, pitch, offset_bytes=0, what=""):
        return self.check(self.dev.get(self.ptr, (self.room,), self.dtype), pitch, offset_bytes, what)

    def check(self, whole, pitch, offset_bytes=0, what=""):
        """whole: the room as it came back.  Everything in front of the body, everything behind it (the last item of the
        room included) and the pitch padding body[:, n:] must still be the sentinel; returns body[:, :n]."""
        assert whole.shape == (self.room,) and offset_bytes % self.dtype.itemsize == 0 and pitch >= self.n, what
        lead = GUARD + offset_bytes // self.dtype.itemsize
        end = lead + self.rows * pitch
        assert end + GUARD <= self.room, what
        body = whole[lead:end].reshape(self.rows, pitch)
        assert (whole[:lead] == self.sentinel).all() and (whole[end:] == self.sentinel).all(), what
        assert (body[:, self.n:] == self.sentinel).all(), what
        return body[:, :self.n]


def staged_input(rows_array, pitch, pad=INPUT_PAD, guard=GUARD, offset=0):
    """the rows (flow or PCM, [rows][n]) at that pitch inside a flat array of pad: guard + offset items in front of them,
    at least guard behind; a launch reads from item guard + offset"""
    rows_array = np.asarray(rows_array)
    r, n = rows_array.shape
    staged = np.full(r * pitch + 2 * guard + 1 + offset, pad, dtype=rows_array.dtype)
    staged[guard + offset:guard + offset + r * pitch].reshape(r, pitch)[:, :n] = rows_array
    return staged


def guarded_plan_launch(eng, lanes, ns, kind=vs.VS_KIND_SYNTH, out_pitch=None, flow=None, in_pitch=None, out_off=0,
                        in_off=0):
    """one launch of a plan into a sentinel-filled buffer: (rows [lanes][ns], kernel name, plan info).  out_off, in_off:
    samples (2 bytes each) added to the output and the input base.  The guard samples in front of and behind the rows
    and the pitch padding must come back untouched."""
    n = len(lanes)
    out_pitch = ns if out_pitch is None else out_pitch
    with eng.scope() as dev:
        plan = dev.plan(lanes, ns)
        name, info = plan.kernel_name(kind), plan.info()
        out = GuardedRows(n, ns, out_pitch, 2 * out_off).on(dev)
        in_ptr = None
        if kind == vs.VS_KIND_FILTER:
            in_pitch = ns if in_pitch is None else in_pitch
            in_ptr = dev.put(staged_input(flow, in_pitch, offset=in_off)) + 2 * (GUARD + in_off)
        plan.launch(kind, out.first(out_pitch, 2 * out_off), out_pitch=out_pitch, in_ptr=in_ptr, in_pitch=in_pitch)
        eng.synchronize()
        assert plan.status() == 0
        rows = out.rows_back(out_pitch, 2 * out_off, (name, n, ns, out_pitch, in_pitch, out_off, in_off))
    return rows, name, info
