"""Session renderer: head-tracked binaural renders of any length, host audio in, host audio out.

The layer above the C ABI that turns the scheduled batch calls into a renderer.  It adds no kernel and no C entry: every sample is
computed by `BatchProcessor`'s existing calls; torch owns the streams, the pinned and the device memory, and does the one elementwise
sum of the late part.

* `HeadTrack`, `nearest_set`, `yaw_rows`: a tracker log in degrees -> rows of table indices per session segment (numpy only).
* `plan_calls`, `call_rows`: the cuts of a stretch of the session into calls of at most `chunk_blocks` blocks, and the rows each call
  runs with (pure Python).
* `SessionRenderer`: the pipeline.  Copy-in of chunk i + 1, the kernels of chunk i and copy-out of chunk i - 1 are queued on three
  streams so that they overlap (measured: tools/bench_session.py); two pinned staging pairs and two device
  pairs of `chunk_blocks` blocks are allocated at construction, so neither device
  nor pinned memory grows with the session.
  `render_pcm` is the same pipeline with integer PCM over the link: the codec of pcm.py runs on the compute stream in front of and
  behind the kernels.
* `render_files`, PCM and tracker-CSV helpers: one WAV per stream, read and written chunk by chunk.
"""
from __future__ import annotations

import math
import queue
import threading
import wave

import numpy as np

from .batch import LAYOUT_5_1, LAYOUT_7_1, BatchProcessor
from .dsp import BLOCK_SIZE
from .pcm import PCM_BITS, WavReader, pcm_decode_device, pcm_dtype, pcm_encode_device, pcm_shape

__all__ = ["HeadTrack", "nearest_set", "yaw_rows", "plan_calls", "call_rows", "SessionRenderer", "render_files", "pcm_decode",
           "pcm_encode", "read_track_csv", "pcm_decode_device", "pcm_encode_device", "WavReader"]


# ---- 1. head tracks to table rows --------------------------------------------------------------------------------------------------
class HeadTrack:
    """A tracker log: yaw_deg[i] (degrees, positive to the right: the convention of set_layout_table_yaws) at times_s[i], strictly
    increasing.  The samples are unwrapped with period 360 once, so a log that crosses +180 -> -180 passes through 180."""

    def __init__(self, times_s, yaw_deg):
        t = np.asarray(times_s, np.float64).reshape(-1)
        y = np.asarray(yaw_deg, np.float64).reshape(-1)
        if t.size == 0 or t.size != y.size:
            raise ValueError("a head track needs as many times as yaws, at least one")
        if not (np.isfinite(t).all() and np.isfinite(y).all()):
            raise ValueError("a head track holds finite numbers")
        if (np.diff(t) <= 0).any():
            raise ValueError("times_s must be strictly increasing")
        self.times_s = t
        self.yaw_deg = np.unwrap(y, period=360.0)

    def at(self, t):
        """the yaw at time(s) t: linear on the unwrapped angle, the first / last value held outside the log (not wrapped back:
        nearest_set takes any angle)"""
        return np.interp(np.asarray(t, np.float64), self.times_s, self.yaw_deg)


def nearest_set(yaw_deg, grid_deg) -> np.ndarray:
    """index of the grid yaw nearest to each yaw on the circle, |((y - g + 180) mod 360) - 180|; the lowest index wins a tie.
    -> uint32, the shape of yaw_deg"""
    y = np.asarray(yaw_deg, np.float64)
    g = np.asarray(grid_deg, np.float64).reshape(-1)
    if g.size == 0:
        raise ValueError("an empty yaw grid")
    d = np.abs(np.mod(y[..., None] - g + 180.0, 360.0) - 180.0)
    return np.argmin(d, axis=-1).astype(np.uint32)


def _seg_range(first_block, n_blocks, seg_blocks):
    return int(first_block) // int(seg_blocks), -(-(int(first_block) + int(n_blocks)) // int(seg_blocks))


def yaw_rows(tracks, first_block, n_blocks, seg_blocks, fs, grid_deg) -> np.ndarray:
    """Rows of set indices for the session segments that session blocks [first_block, first_block + n_blocks) touch.  Segment k
    covers session blocks [k seg_blocks, (k + 1) seg_blocks); its set is nearest_set of the track at its first frame's time,
    k seg_blocks 512 / fs.  tracks: a HeadTrack -> one row [n_segs] for all streams; a sequence of them -> [n_streams][n_segs];
    or plain degrees per segment, [n_segs] or [n_streams][n_segs], entry j for the stretch's j-th segment."""
    k0, k1 = _seg_range(first_block, n_blocks, seg_blocks)
    t = np.arange(k0, k1, dtype=np.float64) * (int(seg_blocks) * BLOCK_SIZE) / float(fs)
    if isinstance(tracks, HeadTrack):
        return nearest_set(tracks.at(t), grid_deg)
    if isinstance(tracks, (list, tuple)) and len(tracks) and all(isinstance(tr, HeadTrack) for tr in tracks):
        return np.stack([nearest_set(tr.at(t), grid_deg) for tr in tracks])
    deg = np.asarray(tracks, np.float64)
    if deg.ndim not in (1, 2) or deg.shape[-1] < k1 - k0:
        raise ValueError(f"yaw in degrees: expected [{k1 - k0}] or [n_streams][{k1 - k0}], got {deg.shape}")
    return nearest_set(deg[..., :k1 - k0], grid_deg)


# ---- 2. the chunk planner ----------------------------------------------------------------------------------------------------------
def plan_calls(first_block, n_blocks, seg_blocks, chunk_blocks):
    """The calls that session blocks [first_block, first_block + n_blocks) are cut into, none longer than chunk_blocks:
    yields (start_block, n_blocks_of_call, call_seg_blocks, repeat).

    The C calls count segments from the call's first block, and only a call's last segment may be short.  So a call runs with
    segments of g = call_seg_blocks blocks, g = gcd(seg_blocks, start_block, and -- for every call but the last -- its length):
    every session boundary inside the call then falls on a boundary of the call, and each session index is repeated
    repeat = seg_blocks / g times (call_rows).  Equal neighbours are no boundary to the kernels, so the fades stay where the
    session puts them."""
    first_block, n_blocks, seg_blocks, chunk_blocks = int(first_block), int(n_blocks), int(seg_blocks), int(chunk_blocks)
    if first_block < 0 or n_blocks < 0 or seg_blocks < 1 or chunk_blocks < 1:
        raise ValueError("plan_calls: first_block, n_blocks >= 0 and seg_blocks, chunk_blocks >= 1")
    pos, end = first_block, first_block + n_blocks
    while pos < end:
        n = min(chunk_blocks, end - pos)
        g = math.gcd(seg_blocks, pos)
        if pos + n < end:
            g = math.gcd(g, n)
        yield pos, n, g, seg_blocks // g
        pos += n


def call_rows(rows, first_seg, start_block, n_blocks, call_seg_blocks, seg_blocks) -> np.ndarray:
    """the rows of one planned call: rows [..., n_segs] holds the session's sets from session segment first_seg on; the call's
    j-th segment of call_seg_blocks blocks takes the set of the session segment its first block lies in"""
    j = np.arange(-(-int(n_blocks) // int(call_seg_blocks)))
    k = (int(start_block) + j * int(call_seg_blocks)) // int(seg_blocks) - int(first_seg)
    return np.ascontiguousarray(np.asarray(rows)[..., k], dtype=np.uint32)


# ---- 3. the renderer ---------------------------------------------------------------------------------------------------------------
class _Slot:
    """one pinned staging pair, one device pair, and the events of the chunk that last used them"""

    def __init__(self, torch, n_in, n_out, device, need_d_out):
        self.h_in = torch.empty(n_in, dtype=torch.float32, pin_memory=True)
        self.h_out = torch.empty(n_out, dtype=torch.float32, pin_memory=True)
        self.d_in = torch.empty(n_in, dtype=torch.float32, device=device)
        self.d_out = torch.empty(n_out, dtype=torch.float32, device=device) if need_d_out else None
        self.ev_in, self.ev_comp, self.ev_out = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        self.pending = None         # (frame offset in `out`, frames) of the chunk whose output is on its way into h_out


class SessionRenderer:
    """Host audio of any length, head yaw per stream -> binaural audio, pipelined over the link.

    Two modes, one constructor each:
      layout(...)  K speaker channels per stream (5.1, 7.1, ...) through a table of layouts per head yaw:
                   BatchProcessor.process_layout_scheduled_ptr, out of place; result = EQ(gain * conv(x)).
      stereo(...)  two speaker channels through a table of sets of four responses: process_ir_crossfaded_ptr (crossfade=False:
                   process_ir_scheduled_ptr under "ring_out"), in place on the device chunk; result = gain * conv(EQ(x)) as in
                   BatchProcessor.process.  An optional static late part, late_irs [4][L] -- tap 512 + k of path p's full response --
                   lives on a second BatchProcessor as zeros(512) ++ late_irs[p], served by the library's long-response plans; both
                   handles read the same device input and the output is head + late, one torch add per chunk.  The setters of this
                   class reach both handles: the EQ is bit-exact, so both convolve the same EQ(x) -- and the EQ RUNS TWICE per
                   chunk.  That is the price of composing the two without a new C entry.

    The session: segment k covers session blocks [k seg_blocks, (k + 1) seg_blocks) (a block is 512 frames) and has one set per
    stream; where a stream's set changes, the first block of the new segment fades from the old set (crossfade=False: the old set's
    tail rings out under the new one).  render() may be called again and again: the position and every stream's last set persist,
    and the bits do not depend on where the session is cut into render() calls, nor -- in layout mode -- on chunk_blocks.

    `.batch` is the underlying processor (`.late_batch` the late part's, or None).  Setters that must reach both are methods here.
    Device and pinned memory are allocated once, for chunk_blocks blocks; nothing grows with the session."""

    def __init__(self, mode, n_streams, channels, yaw_grid, *, seg_blocks=2, chunk_blocks=64, crossfade=True, fs=48000.0,
                 num_bands=10, device=0, late_len=0, library=None):
        import torch
        if mode not in ("layout", "stereo"):
            raise ValueError("mode is 'layout' or 'stereo'")
        if int(n_streams) < 1 or int(seg_blocks) < 1 or int(chunk_blocks) < 1 or not float(fs) > 0:
            raise ValueError("n_streams, seg_blocks, chunk_blocks >= 1 and fs > 0")
        self.mode, self.n_streams, self.channels = mode, int(n_streams), int(channels)
        self.yaw_grid = np.asarray(yaw_grid, np.float64).reshape(-1)
        self.seg_blocks, self.chunk_blocks, self.crossfade, self.fs = int(seg_blocks), int(chunk_blocks), bool(crossfade), float(fs)
        self.device = int(device)
        self.reach = 0
        self.batch = BatchProcessor(self.n_streams, num_bands, self.device, library)
        self.late_batch = BatchProcessor(self.n_streams, num_bands, self.device, library) if late_len else None
        self._torch = torch
        self._dev = torch.device("cuda", self.device)
        chunk = self.chunk_blocks * BLOCK_SIZE
        with torch.cuda.device(self._dev):
            self._s_in, self._s_comp, self._s_out = (torch.cuda.Stream(self._dev) for _ in range(3))
            need_d_out = mode == "layout" or late_len > 0
            self._slots = [_Slot(torch, self.n_streams * self.channels * chunk, self.n_streams * 2 * chunk, self._dev, need_d_out)
                           for _ in range(2)]
        self._turn = 0              # chunks rendered so far: the slot of the next one is _turn % 2
        self._pos = 0               # session position in blocks
        self._last = None           # every stream's last set [n_streams], None at the session's start
        self._finished = False
        self._broken = False        # a render() failed behind its first queued chunk: the handles' state is ahead of _pos
        self._pcm = None            # render_pcm's device buffers, allocated by its first call
        self._bytes_in = self._bytes_out = 0

    # -- constructors ---------------------------------------------------------------------
    @classmethod
    def layout(cls, n_streams, table, yaw_grid, *, late_irs=None, seg_blocks=2, chunk_blocks=64, crossfade=True, fs=48000.0,
               num_bands=10, device=0, library=None):
        """table [n_sets][K][2][len <= 512], set j the layout at head yaw yaw_grid[j] (degrees)"""
        if late_irs is not None:
            raise ValueError("a late part is available in stereo mode only")
        table = np.asarray(table, np.float32)
        grid = np.asarray(yaw_grid, np.float64).reshape(-1)
        if table.ndim != 4 or table.shape[2] != 2 or table.shape[0] != grid.size or table.size == 0:
            raise ValueError(f"expected table [{grid.size}][K][2][len], got {table.shape}")
        r = cls("layout", n_streams, table.shape[1], grid, seg_blocks=seg_blocks, chunk_blocks=chunk_blocks, crossfade=crossfade,
                fs=fs, num_bands=num_bands, device=device, library=library)
        r.batch.set_layout_table(table)
        r.reach = table.shape[3] - 1
        return r

    @classmethod
    def layout_from_sofa(cls, n_streams, sofa, layout, yaw_grid, *, radius_m=1.0, late_irs=None, seg_blocks=2, chunk_blocks=64,
                         crossfade=True, fs=48000.0, num_bands=10, device=0, library=None):
        """layout: a preset such as LAYOUT_5_1 or (name, azimuth, elevation) rows; the table is set_layout_table_yaws' (resampled
        to fs where the file's rate differs)"""
        if late_irs is not None:
            raise ValueError("a late part is available in stereo mode only")
        grid = np.asarray(yaw_grid, np.float64).reshape(-1)
        r = cls("layout", n_streams, len(layout), grid, seg_blocks=seg_blocks, chunk_blocks=chunk_blocks, crossfade=crossfade,
                fs=fs, num_bands=num_bands, device=device, library=library)
        table = r.batch.set_layout_table_yaws(sofa, layout, grid, radius_m=radius_m, fs=r.fs)
        r.reach = table.shape[3] - 1
        return r

    @classmethod
    def stereo(cls, n_streams, sets, yaw_grid, *, late_irs=None, seg_blocks=2, chunk_blocks=64, crossfade=True, fs=48000.0,
               num_bands=10, device=0, library=None):
        """sets [n_sets][4][len <= 512] = [Lsl, Lsr, Rsl, Rsr] at head yaw yaw_grid[j]; late_irs [4][L] or None"""
        sets = np.asarray(sets, np.float32)
        grid = np.asarray(yaw_grid, np.float64).reshape(-1)
        if sets.ndim != 3 or sets.shape[1] != 4 or sets.shape[0] != grid.size or sets.size == 0:
            raise ValueError(f"expected sets [{grid.size}][4][len], got {sets.shape}")
        late = cls._check_late(late_irs)
        r = cls("stereo", n_streams, 2, grid, seg_blocks=seg_blocks, chunk_blocks=chunk_blocks, crossfade=crossfade, fs=fs,
                num_bands=num_bands, device=device, late_len=0 if late is None else late.shape[1], library=library)
        r.batch.set_schedule_irs(sets)
        r._set_late(late, sets.shape[2])
        return r

    @classmethod
    def stereo_from_sofa(cls, n_streams, sofa, yaw_grid, *, az_l=-30.0, el_l=0.0, az_r=30.0, el_r=0.0, radius_m=1.0,
                         late_irs=None, seg_blocks=2, chunk_blocks=64, crossfade=True, fs=48000.0, num_bands=10, device=0,
                         library=None):
        """two speakers at the plugin's angles; set j is set_schedule_speakers' on (az_l - yaw_j, el_l, az_r - yaw_j, el_r), the
        azimuths wrapped to (-180, 180]"""
        grid = np.asarray(yaw_grid, np.float64).reshape(-1)
        late = cls._check_late(late_irs)
        r = cls("stereo", n_streams, 2, grid, seg_blocks=seg_blocks, chunk_blocks=chunk_blocks, crossfade=crossfade, fs=fs,
                num_bands=num_bands, device=device, late_len=0 if late is None else late.shape[1], library=library)

        def wrap(a):
            return -(np.mod(-a + 180.0, 360.0) - 180.0)

        angles = np.stack([wrap(az_l - grid), np.full(grid.size, float(el_l)), wrap(az_r - grid), np.full(grid.size, float(el_r))],
                          axis=1)
        sets = r.batch.set_schedule_speakers(sofa, angles, radius_m, r.fs)
        r._set_late(late, sets.shape[2])
        return r

    @staticmethod
    def _check_late(late_irs):
        if late_irs is None:
            return None
        late = np.asarray(late_irs, np.float32)
        if late.ndim != 2 or late.shape[0] != 4 or late.shape[1] == 0:
            raise ValueError(f"expected late_irs [4][L], got {late.shape}")
        return late

    def _set_late(self, late, head_len):
        self.reach = head_len - 1
        if late is None:
            return
        full = np.concatenate([np.zeros((4, BLOCK_SIZE), np.float32), late], axis=1)
        for p in range(4):
            self.late_batch.set_ir(p, full[p])
        self.reach = full.shape[1] - 1

    # -- setters that reach both handles ---------------------------------------------------
    def _both(self):
        return [self.batch] if self.late_batch is None else [self.batch, self.late_batch]

    def set_gain(self, gain):
        for b in self._both():
            b.set_gain(gain)

    def set_eq_enabled(self, eq_enable):
        for b in self._both():
            b.set_eq_enabled(eq_enable)

    def set_band_coeffs(self, band_idx, coeffs, enabled):
        for b in self._both():
            b.set_band_coeffs(band_idx, coeffs, enabled)

    def update_band_coeffs(self, band_idx, sample_rate, config):
        for b in self._both():
            b.update_band_coeffs(band_idx, sample_rate, config)

    def set_stream_band_coeffs(self, stream, band_idx, coeffs, enabled):
        for b in self._both():
            b.set_stream_band_coeffs(stream, band_idx, coeffs, enabled)

    def update_stream_band_coeffs(self, stream, band_idx, sample_rate, config):
        for b in self._both():
            b.update_stream_band_coeffs(stream, band_idx, sample_rate, config)

    def share_eq_table(self):
        for b in self._both():
            b.share_eq_table()

    # -- the session ------------------------------------------------------------------------
    @property
    def position_blocks(self):
        return self._pos

    def reset(self):
        """restart the session: position 0, no last set, BatchProcessor.reset on the handle(s)"""
        self._torch.cuda.synchronize(self._dev)
        for b in self._both():
            b.reset()
        for sl in self._slots:
            sl.pending = None
        self._pos, self._last, self._finished, self._broken = 0, None, False, False
        self._bytes_in = self._bytes_out = 0

    def _rows_of_call(self, yaw, rows, n_blocks, n_given):
        """the validated session rows of this call, [n_segs] or [n_streams][n_segs]: n_given segments must be there, the segments
        that hold padding and ring-out only take the last value"""
        n_segs = -(-n_blocks // self.seg_blocks)
        if yaw is not None:
            if isinstance(yaw, HeadTrack) or (isinstance(yaw, (list, tuple)) and len(yaw) and isinstance(yaw[0], HeadTrack)):
                if not isinstance(yaw, HeadTrack) and len(yaw) != self.n_streams:
                    raise ValueError(f"expected one track or {self.n_streams}, got {len(yaw)}")
                return yaw_rows(yaw, self._pos, n_blocks, self.seg_blocks, self.fs, self.yaw_grid)
            deg = np.asarray(yaw, np.float64)
            a = nearest_set(deg, self.yaw_grid) if deg.ndim in (1, 2) else deg
            what = "yaw"
        else:
            a = np.asarray(rows)
            if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() >= self.yaw_grid.size):
                raise ValueError(f"rows holds indices 0 .. {self.yaw_grid.size - 1}")
            a = a.astype(np.uint32)
            what = "rows"
        if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[0] != self.n_streams) or a.shape[-1] < max(n_given, 1):
            raise ValueError(f"{what}: expected [>= {n_given}] or [{self.n_streams}][>= {n_given}], got {a.shape}")
        a = a[..., :n_segs]
        if a.shape[-1] < n_segs:
            a = np.concatenate([a, np.repeat(a[..., -1:], n_segs - a.shape[-1], axis=-1)], axis=-1)
        return np.ascontiguousarray(a)

    def render(self, x, yaw=None, rows=None, prev=None, final=False, ring_out=False, out=None):
        """x: HOST audio [n_streams][K or 2][frames], numpy or a torch host tensor, float32 -> [n_streams][2][frames] of the same kind
        (`out` if given).  Blocking: the result is complete on return.

        yaw or rows, exactly one: yaw is a HeadTrack (all streams), a sequence of n_streams HeadTracks, or degrees per session
        segment of this call, [n_segs] or [n_streams][n_segs]; rows holds table indices in the same shapes.  prev: the set(s) in
        front of the session's first block (a scalar or [n_streams]); at the session's start only.
        frames must be a multiple of seg_blocks * 512 unless final=True; a final call may be ragged -- its input is zero-padded to a
        block, its output trimmed -- and with ring_out=True the response's reach (`.reach` frames) is appended as silence and
        returned as well.  Segments that hold only padding keep the last given value.  After a final call the session is over until
        reset().

        A pinned torch tensor is copied to the device as it is where the call is one chunk (its chunk slice is then contiguous);
        every other input goes through the pinned staging buffers."""
        torch = self._torch
        is_np = isinstance(x, np.ndarray)
        if not is_np and not isinstance(x, torch.Tensor):
            x = np.asarray(x, np.float32)
            is_np = True
        self._check_session(yaw, rows)
        if x.ndim != 3 or x.shape[0] != self.n_streams or x.shape[1] != self.channels:
            raise ValueError(f"expected x [{self.n_streams}][{self.channels}][frames], got {tuple(x.shape)}")
        if (x.dtype != np.float32) if is_np else (x.dtype != torch.float32 or x.is_cuda):
            raise TypeError("x must be float32 host audio")
        frames = int(x.shape[2])
        out_frames, n_blocks, sess_rows, last = self._plan_call(frames, yaw, rows, prev, final, ring_out)
        if out is None:
            out = np.empty((self.n_streams, 2, out_frames), np.float32) if is_np else torch.empty((self.n_streams, 2, out_frames), dtype=torch.float32)
        elif tuple(out.shape) != (self.n_streams, 2, out_frames) or isinstance(out, np.ndarray) != is_np \
                or (out.dtype != np.float32 if is_np else (out.dtype != torch.float32 or out.is_cuda)):
            raise ValueError(f"out: a float32 host array [{self.n_streams}][2][{out_frames}] of x's kind")
        if n_blocks == 0:
            return out
        xt = torch.from_numpy(x) if is_np else x
        ot = torch.from_numpy(out) if is_np else out
        self._run(xt, ot, frames, out_frames, n_blocks, sess_rows, last, final, None)
        return out

    def render_pcm(self, x, yaw=None, rows=None, prev=None, final=False, ring_out=False, out=None, out_bits=None):
        """render() on integer PCM, with integers over the link.  x: HOST PCM in WAV frame order, numpy or a torch host tensor:
        int16 [n_streams][frames][K or 2] (16-bit), int32 of that shape (32-bit) or uint8 [n_streams][frames][K or 2][3] (24-bit,
        packed, little-endian) -> [n_streams][out_frames][2] of the same kind, of the out_bits kind (16, 24 or 32) when given, or
        `out` when given and of exactly that kind and shape.  Blocking.

        Bit for bit, per stream, pcm_encode(render(pcm_decode(x)), out_bits) with the same yaw / rows / prev / final / ring_out:
        everything render() documents holds, and the two may alternate within one session -- position, last set and the handles'
        state are shared.  Decode is int / 2^(bits - 1); encode is round-half-even, clip, no dither.

        The pipeline is render()'s: the chunk's frames are copied as PCM bytes into the slot's pinned staging buffer (the float one,
        viewed as bytes: PCM is never wider), copy-in lands them in a device PCM buffer, pcm_decode_device writes the slot's float
        input on the compute stream in front of the kernels (frames behind the input's end are zeroed there and never cross the
        link), pcm_encode_device writes the device PCM output behind them, copy-out moves those bytes and the drain copies them
        into the result.  A pinned tensor whose chunk slice is contiguous (a call of one chunk) is copied to the device as it is.

        Memory: the first render_pcm() allocates, once and for the widest format, two device PCM pairs and the codec's scratch
        (an int32 word per input sample for 24-bit input; a float64 and an int32 word per output sample):
        (12 C + 40) S chunk_blocks 512 bytes on top of render()'s (8 C + 16) S chunk_blocks 512, (20 C + 56) S chunk_blocks 512
        in all; no pinned memory is added.  A renderer that only calls render() allocates what it always did."""
        torch = self._torch
        is_np = isinstance(x, np.ndarray)
        if not is_np and not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            is_np = True
        self._check_session(yaw, rows)
        bits = self._pcm_kind(x, is_np, "x", self.channels)
        frames = int(x.shape[1])
        if out_bits is None:
            out_bits = bits
        elif out_bits not in PCM_BITS:
            raise ValueError(f"out_bits {out_bits!r}: 16, 24 or 32")
        out_frames, n_blocks, sess_rows, last = self._plan_call(frames, yaw, rows, prev, final, ring_out)
        shape = pcm_shape(out_bits, self.n_streams, out_frames, 2)
        if out is None:
            out = np.empty(shape, pcm_dtype(np, out_bits)) if is_np else torch.empty(shape, dtype=pcm_dtype(torch, out_bits))
        elif isinstance(out, np.ndarray) != is_np or not (is_np or isinstance(out, torch.Tensor)) or tuple(out.shape) != shape \
                or self._pcm_kind(out, is_np, "out", 2) != out_bits:
            raise ValueError(f"out: {out_bits}-bit host PCM {shape} of x's kind")
        if n_blocks == 0:
            return out
        if self._pcm is None:
            with torch.cuda.stream(self._s_comp):       # the stream that decodes: the fill of word_in is ordered in front of it
                self._pcm = _PcmBuffers(torch, self.n_streams, self.channels, self.chunk_blocks * BLOCK_SIZE, self._dev)
        xt = torch.from_numpy(x) if is_np else x
        ot = torch.from_numpy(out) if is_np else out
        self._run(xt, ot, frames, out_frames, n_blocks, sess_rows, last, final, (bits, out_bits))
        return out

    @property
    def link_bytes(self):
        """(bytes_in, bytes_out) queued over the link since construction or reset(), by render() and render_pcm() alike: what the
        copies really carry.  render() moves every chunk whole, zero padding and ring-out included, four bytes per sample;
        render_pcm() moves the frames the input holds in and the frames that are kept out.  So on calls of whole blocks without
        ring-out the 16-bit figures are exactly half of render()'s and the 24-bit ones three quarters; on a ragged or ring-out
        call render_pcm() moves less than that."""
        return self._bytes_in, self._bytes_out

    def _pcm_kind(self, a, is_np, what, channels):
        """the sample width of host PCM `a`, [n_streams][frames][channels] int16 / int32 or [...][3] uint8"""
        torch = self._torch
        if (np.issubdtype(a.dtype, np.floating) if is_np else a.dtype.is_floating_point):
            raise TypeError(f"{what}: integer PCM; float audio is render()'s")
        if not is_np and a.is_cuda:
            raise TypeError(f"{what} must be host PCM")
        i16, i32, u8 = (np.int16, np.int32, np.uint8) if is_np else (torch.int16, torch.int32, torch.uint8)
        if a.ndim == 3 and a.dtype in (i16, i32):
            bits = 16 if a.dtype == i16 else 32
        elif a.ndim == 4 and a.dtype == u8 and a.shape[3] == 3:
            bits = 24
        else:
            raise ValueError(f"{what}: int16 or int32 [n_streams][frames][channels], or uint8 [n_streams][frames][channels][3]; "
                             f"got {a.dtype} {tuple(a.shape)}")
        if a.shape[0] != self.n_streams or a.shape[2] != channels:
            raise ValueError(f"expected {what} [{self.n_streams}][frames][{channels}], got {tuple(a.shape)}")
        return bits

    def _check_session(self, yaw, rows):
        if self._finished:
            raise ValueError("the session ended with a final call: reset() starts the next one")
        if self._broken:
            raise RuntimeError("an earlier render() failed midway, the handles' state is undefined: reset() starts a new session")
        if (yaw is None) == (rows is None):
            raise ValueError("give either yaw or rows")

    def _plan_call(self, frames, yaw, rows, prev, final, ring_out):
        """the checks of a call of `frames` frames that do not depend on the samples' format -> (out_frames, n_blocks, the session
        rows of the call, every stream's set in front of it or None)"""
        if ring_out and not final:
            raise ValueError("ring_out belongs to the final call")
        if not final and frames % (self.seg_blocks * BLOCK_SIZE):
            raise ValueError(f"a call that is not final holds a multiple of {self.seg_blocks * BLOCK_SIZE} frames, got {frames}")
        if prev is not None and self._pos:
            raise ValueError("prev names the set in front of the session's first block")
        out_frames = frames + (self.reach if ring_out else 0)
        n_blocks = -(-out_frames // BLOCK_SIZE)
        sess_rows = self._rows_of_call(yaw, rows, n_blocks, -(-frames // (self.seg_blocks * BLOCK_SIZE)))
        last = self._last
        if prev is not None:
            pv = np.asarray(prev).reshape(-1)
            if pv.size not in (1, self.n_streams) or pv.min() < 0 or pv.max() >= self.yaw_grid.size:
                raise ValueError(f"prev: one index or {self.n_streams}, each below {self.yaw_grid.size}")
            last = np.broadcast_to(pv.astype(np.uint32), (self.n_streams,)).copy()
        return out_frames, n_blocks, sess_rows, last

    def _run(self, xt, ot, frames, out_frames, n_blocks, sess_rows, last, final, fmt):
        """queue the planned calls of one render() / render_pcm() (fmt: None or (bits in, bits out)), drain, advance the session"""
        # one row for all streams stays one row (the kernels' cheapest case) while every stream has the same set in front of it
        if sess_rows.ndim == 1 and last is not None and (last != last[0]).any():
            sess_rows = np.ascontiguousarray(np.broadcast_to(sess_rows, (self.n_streams, sess_rows.size)))
        first_seg = self._pos // self.seg_blocks
        try:
            for start, n, g, _ in plan_calls(self._pos, n_blocks, self.seg_blocks, self.chunk_blocks):
                idx = call_rows(sess_rows, first_seg, start, n, g, self.seg_blocks)
                if start > self._pos:
                    pv = sess_rows[..., (start - 1) // self.seg_blocks - first_seg]
                else:
                    pv = None if last is None else (last if sess_rows.ndim == 2 else last[0])
                self._chunk(xt, ot, (start - self._pos) * BLOCK_SIZE, n, g, idx, pv, frames, out_frames, fmt)
            self._drain_all(ot)
        except BaseException:
            self._broken = True                         # overlaps and EQ state are ahead of _pos and _last
            self._torch.cuda.synchronize(self._dev)
            for sl in self._slots:
                sl.pending = None
            raise
        self._pos += n_blocks
        self._last = np.broadcast_to(sess_rows[..., -1], (self.n_streams,)).astype(np.uint32)
        self._finished = bool(final)

    # -- the pipeline -----------------------------------------------------------------------
    def _chunk(self, xt, ot, f0, n_blocks, g, idx, prev, in_frames, out_frames, fmt):
        """queue one planned call: frames [f0, f0 + n_blocks 512) of this render() call"""
        torch = self._torch
        S, C = self.n_streams, self.channels
        n = n_blocks * BLOCK_SIZE
        turn = self._turn % 2
        sl = self._slots[turn]
        self._turn += 1
        have = max(0, min(n, in_frames - f0))          # frames of x in this chunk; the rest is padding and ring-out
        keep = max(0, min(n, out_frames - f0))
        d_in = sl.d_in[:S * C * n].view(S, C, n)
        in_place = sl.d_out is None
        d_res = d_in if in_place else sl.d_out[:S * 2 * n].view(S, 2, n)
        if fmt is None:
            self._copy_in(sl, xt[:, :, f0:f0 + have], d_in, have, in_place)
        else:
            pb = self._pcm
            w_out = fmt[1] // 8
            raw = self._copy_in_pcm(sl, turn, xt[:, f0:f0 + have], have, fmt[0])
        with torch.cuda.stream(self._s_comp):
            self._s_comp.wait_event(sl.ev_in)
            self._s_comp.wait_event(sl.ev_out)          # the copy-out that last read d_out (the device PCM output) is done
            if fmt is not None:
                if have:
                    word = pb.word_in[:S * have * C].view(S, have, C) if fmt[0] == 24 else None
                    pcm_decode_device(raw, fmt[0], d_in[:, :, :have], word)
                if have < n:
                    d_in[:, :, have:].zero_()
                pb.ev_dec[turn].record(self._s_comp)
            hs = self._s_comp.cuda_stream
            if self.mode == "layout":
                self.batch.process_layout_scheduled_ptr(d_in.data_ptr(), d_res.data_ptr(), n_blocks, C * n, n, 2 * n, n, g, idx,
                                                        prev if self.crossfade else None, self.crossfade, hs)
            else:
                if self.late_batch is not None:         # first: it reads the input the head then overwrites
                    self.late_batch.process_ptr(d_in.data_ptr(), d_res.data_ptr(), n_blocks, 2 * n, n, hs)
                if self.crossfade:
                    self.batch.process_ir_crossfaded_ptr(d_in.data_ptr(), d_in.data_ptr(), n_blocks, 2 * n, n, g, idx, prev, hs)
                else:
                    self.batch.process_ir_scheduled_ptr(d_in.data_ptr(), d_in.data_ptr(), n_blocks, 2 * n, n, g, idx, "ring_out", hs)
                if self.late_batch is not None:
                    d_res.add_(d_in)
            if fmt is not None and keep:
                d_pcm = pb.d_out[turn][:S * keep * 2 * w_out].view(pcm_dtype(torch, fmt[1])).view(pcm_shape(fmt[1], S, keep, 2))
                pcm_encode_device(d_res[:, :, :keep], fmt[1], d_pcm, pb.f64[:S * 2 * keep].view(S, 2, keep),
                                  pb.word_out[:S * keep * 2].view(S, keep, 2) if fmt[1] == 24 else None)
            sl.ev_comp.record(self._s_comp)
        self._drain(sl, ot)                             # h_out still holds the chunk two turns back
        with torch.cuda.stream(self._s_out):
            self._s_out.wait_event(sl.ev_comp)
            if fmt is None:
                sl.h_out[:S * 2 * n].copy_(d_res.reshape(-1), non_blocking=True)
                self._bytes_out += 4 * S * 2 * n
            elif keep:
                nb = S * keep * 2 * w_out
                sl.h_out.view(torch.uint8)[:nb].copy_(pb.d_out[turn][:nb], non_blocking=True)
                self._bytes_out += nb
            sl.ev_out.record(self._s_out)
        sl.pending = (f0, n, keep, None if fmt is None else fmt[1])

    def _copy_in(self, sl, src, d_in, have, in_place):
        """float audio: the chunk's slice of x, zero-padded to the chunk, into the slot's device input"""
        S, C, n = d_in.shape
        direct = have == n and src.is_contiguous() and src.is_pinned()
        if not direct:
            sl.ev_in.synchronize()                      # the copy that last read h_in is done
            h_in = sl.h_in[:S * C * n].view(S, C, n)
            h_in[:, :, :have].copy_(src)
            if have < n:
                h_in[:, :, have:].zero_()
            src = h_in
        with self._torch.cuda.stream(self._s_in):
            self._s_in.wait_event(sl.ev_comp)           # the kernels that last read d_in are done
            if in_place:
                self._s_in.wait_event(sl.ev_out)        # ... and so is the copy-out of what they left there
            d_in.copy_(src, non_blocking=True)
            sl.ev_in.record(self._s_in)
        self._bytes_in += 4 * S * C * n

    def _copy_in_pcm(self, sl, turn, src, have, bits):
        """PCM: the `have` frames of x in this chunk, as they are, into the slot's device PCM input -> that input's view"""
        torch = self._torch
        S, C = self.n_streams, self.channels
        nb = S * have * C * (bits // 8)
        raw = self._pcm.d_in[turn][:nb].view(pcm_dtype(torch, bits)).view(pcm_shape(bits, S, have, C))
        if have and not (src.is_contiguous() and src.is_pinned()):
            sl.ev_in.synchronize()                      # the copy that last read h_in is done
            h_in = sl.h_in.view(torch.uint8)[:nb].view(raw.dtype).view(raw.shape)
            h_in.copy_(src)
            src = h_in
        with torch.cuda.stream(self._s_in):
            if have:
                self._s_in.wait_event(self._pcm.ev_dec[turn])       # the decode that last read the device PCM input is done
                raw.copy_(src, non_blocking=True)
            sl.ev_in.record(self._s_in)
        self._bytes_in += nb
        return raw

    def _drain(self, sl, ot):
        if sl.pending is None:
            return
        f0, n, keep, bits = sl.pending
        sl.pending = None
        sl.ev_out.synchronize()
        S = self.n_streams
        if not keep:
            return
        if bits is None:
            ot[:, :, f0:f0 + keep].copy_(sl.h_out[:S * 2 * n].view(S, 2, n)[:, :, :keep])
        else:
            ot[:, f0:f0 + keep].copy_(sl.h_out.view(self._torch.uint8)[:S * keep * 2 * (bits // 8)].view(ot.dtype)
                                      .view(pcm_shape(bits, S, keep, 2)))

    def _drain_all(self, ot):
        for k in (self._turn, self._turn + 1):          # the older chunk first
            self._drain(self._slots[k % 2], ot)


class _PcmBuffers:
    """what render_pcm adds to the two slots, sized for 32-bit samples: a device PCM pair and a decode event per slot; one int32
    word per input sample (24-bit decode; its low bytes stay zero), one float64 and one int32 word per output sample (encode).
    The scratch is touched on the compute stream only, so one copy serves both slots.  Built with the compute stream current:
    the zero fill of word_in is then in front of the first decode in stream order."""

    def __init__(self, torch, S, C, chunk, device):
        self.d_in = [torch.empty(4 * S * C * chunk, dtype=torch.uint8, device=device) for _ in range(2)]
        self.d_out = [torch.empty(4 * S * 2 * chunk, dtype=torch.uint8, device=device) for _ in range(2)]
        self.ev_dec = [torch.cuda.Event(), torch.cuda.Event()]
        self.word_in = torch.zeros(S * C * chunk, dtype=torch.int32, device=device)
        self.f64 = torch.empty(S * 2 * chunk, dtype=torch.float64, device=device)
        self.word_out = torch.empty(S * 2 * chunk, dtype=torch.int32, device=device)


# ---- 4. files ----------------------------------------------------------------------------------------------------------------------
def pcm_decode(data: bytes, bits: int, channels: int) -> np.ndarray:
    """little-endian signed PCM frames -> float32 [channels][frames], value = int / 2^(bits - 1)"""
    if bits not in PCM_BITS:
        raise ValueError(f"PCM of {bits} bits: 16, 24 or 32 are read")
    if bits == 24:
        b = np.frombuffer(data, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = v - ((v & 0x800000) << 1)
    else:
        v = np.frombuffer(data, "<i2" if bits == 16 else "<i4")
    return np.ascontiguousarray((v.astype(np.float64) / float(1 << (bits - 1))).astype(np.float32).reshape(-1, channels).T)


def pcm_encode(x, bits: int) -> bytes:
    """float [channels][frames] -> little-endian signed PCM frames: x 2^(bits - 1) rounded half to even, clipped to
    [-2^(bits - 1), 2^(bits - 1) - 1]; no dither"""
    if bits not in PCM_BITS:
        raise ValueError(f"PCM of {bits} bits: 16, 24 or 32 are written")
    full = float(1 << (bits - 1))
    v = np.clip(np.rint(np.asarray(x, np.float64).T * full), -full, full - 1.0).astype(np.int64).reshape(-1)
    if bits == 16:
        return v.astype("<i2").tobytes()
    if bits == 32:
        return v.astype("<i4").tobytes()
    u = (v & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def read_wav(path):
    """a whole PCM WAV -> (float32 [channels][frames], rate, bits)"""
    with WavReader(path) as w:
        return pcm_decode(w.readframes(w.frames), w.bits, w.channels), w.rate, w.bits


def write_wav(path, x, rate, bits=16):
    """float [channels][frames] -> a PCM WAV (pcm_encode)"""
    x = np.asarray(x)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(x.shape[0])
        w.setsampwidth(bits // 8)
        w.setframerate(int(round(rate)))
        w.writeframes(pcm_encode(x, bits))


def read_track_csv(path) -> HeadTrack:
    """lines of `time_s,yaw_deg` (blank lines, lines starting with # and one header line without numbers are skipped)"""
    t, y = [], []
    with open(path) as f:
        for n, line in enumerate(f):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            a = line.split(",")
            try:
                t0, y0 = float(a[0]), float(a[1])
            except (ValueError, IndexError):
                if not t and n == 0:
                    continue
                raise ValueError(f"{path}: line {n + 1}: expected time_s,yaw_deg")
            t.append(t0)
            y.append(y0)
    return HeadTrack(t, y)


CALL_CHUNKS = 4     # chunks per render() call of render_files


def render_files(inputs, outputs, renderer, tracks=None, ring_out=True, out_bits=None, pcm=None):
    """One PCM WAV per stream (16 / 24 / 32-bit integer; format tag 1 or WAVE_FORMAT_EXTENSIBLE: pcm.WavReader) through `renderer`,
    from the session's start (it is reset first).  All files have the renderer's rate and channel count; lengths may differ:
    shorter files are padded with silence (a track holds its last value behind its log) and each output is trimmed to its own
    length, plus the reach when ring_out.  The outputs are two-channel files (stdlib `wave`) of out_bits (16, 24 or 32) per sample;
    None: of their input's sample width.  tracks: None (yaw 0), one HeadTrack, or one per stream.

    Decode is int / 2^(bits - 1); encode is round-half-even, clip, NO dither (pcm_encode).  Files are read and written
    CALL_CHUNKS * chunk_blocks blocks at a time: host memory does not hold a session either.  -> frames written per output.

    pcm: None -- where all inputs share one sample width, the file bytes go as they are through render_pcm (the codec runs on the
    device, a reader thread fetches the next call's frames and a writer thread writes the previous call's output while the
    current call renders; at most two calls' worth of PCM per direction is held); inputs of mixed widths take the float path.
    False: the float path, always: pcm_decode and pcm_encode on the host around render().  True: the PCM path; mixed widths are
    a ValueError.  Both paths write the same bytes."""
    S = renderer.n_streams
    if len(inputs) != S or len(outputs) != S:
        raise ValueError(f"one input and one output per stream: {S}")
    if out_bits is not None and out_bits not in PCM_BITS:
        raise ValueError(f"out_bits {out_bits!r}: 16, 24 or 32")
    if tracks is None:
        tracks = HeadTrack([0.0], [0.0])
    ins, outs = [], []
    try:
        for p in inputs:
            w = WavReader(p)
            ins.append(w)
            if w.rate != renderer.fs:
                raise ValueError(f"{p}: rate {w.rate}, the renderer runs at {renderer.fs:g}")
            if w.channels != renderer.channels:
                raise ValueError(f"{p}: {w.channels} channels, the renderer takes {renderer.channels}")
        lens = [w.frames for w in ins]
        total = max(lens)
        if total == 0:
            raise ValueError("the inputs are empty")
        one_width = len({w.bits for w in ins}) == 1
        if pcm and not one_width:
            raise ValueError("pcm=True: the inputs hold samples of different widths")
        reach = renderer.reach if ring_out else 0
        for p, w in zip(outputs, ins):
            o = wave.open(str(p), "wb")
            outs.append(o)
            o.setnchannels(2)
            o.setsampwidth((out_bits or w.bits) // 8)
            o.setframerate(w.rate)
        renderer.reset()
        seg = renderer.seg_blocks
        call_frames = max(1, CALL_CHUNKS * renderer.chunk_blocks // seg) * seg * BLOCK_SIZE
        if one_width and (pcm or pcm is None):
            return _render_files_pcm(ins, outs, renderer, tracks, ring_out, lens, reach, call_frames, out_bits or ins[0].bits)
        x = np.zeros((S, renderer.channels, call_frames), np.float32)
        pos, written = 0, [0] * S
        while pos < total:
            n = min(call_frames, total - pos)
            final = pos + n == total
            for s, w in enumerate(ins):
                have = max(0, min(n, lens[s] - pos))
                if have:
                    x[s, :, :have] = pcm_decode(w.readframes(have), w.bits, renderer.channels)
                x[s, :, have:n] = 0.0
            y = renderer.render(x[:, :, :n], yaw=tracks, final=final, ring_out=final and ring_out)
            for s, o in enumerate(outs):
                k = max(0, min(y.shape[2], lens[s] + reach - pos))
                if k:
                    o.writeframes(pcm_encode(y[s, :, :k], 8 * o.getsampwidth()))
                    written[s] += k
            pos += n
        return written
    finally:
        for w in ins + outs:
            w.close()


def _render_files_pcm(ins, outs, renderer, tracks, ring_out, lens, reach, call_frames, out_bits):
    """render_files through render_pcm.  Two host PCM arrays per direction go round: the reader thread fills one with the next
    call's frames while the other renders; the writer thread empties one while the next call fills the other."""
    S, C, bits, total = renderer.n_streams, renderer.channels, ins[0].bits, max(lens)
    xs = [np.zeros(pcm_shape(bits, S, call_frames, C), pcm_dtype(np, bits)) for _ in range(2)]
    ys = [np.empty(pcm_shape(out_bits, S, call_frames + reach, 2), pcm_dtype(np, out_bits)) for _ in range(2)]
    calls = [(pos, min(call_frames, total - pos)) for pos in range(0, total, call_frames)]
    free_x, full_x, free_y, full_y = (queue.Queue() for _ in range(4))
    for i in range(2):
        free_x.put(i)
        free_y.put(i)
    errors, written = [], [0] * S

    def reader():
        try:
            for pos, n in calls:
                i = free_x.get()
                if i is None:
                    return
                for s, w in enumerate(ins):
                    have = max(0, min(n, lens[s] - pos))
                    if have and w.readinto(xs[i][s, :have], have) != have:
                        raise ValueError(f"stream {s}: the file holds fewer frames than its header names")
                    xs[i][s, have:n] = 0
                full_x.put(i)
        except BaseException as e:
            errors.append(e)
            full_x.put(None)

    def writer():
        failed = False
        while True:
            job = full_y.get()
            if job is None:
                return
            i, pos, frames = job
            try:
                for s, o in enumerate(outs):
                    k = max(0, min(frames, lens[s] + reach - pos))
                    if k and not failed:
                        o.writeframes(ys[i][s, :k])
                        written[s] += k
            except BaseException as e:              # keep handing the arrays back, so that the renderer never waits for ever
                failed = True
                errors.append(e)
            free_y.put(i)

    threads = [threading.Thread(target=reader, name="render_files reader"), threading.Thread(target=writer, name="render_files writer")]
    for t in threads:
        t.start()
    try:
        for pos, n in calls:
            i = full_x.get()
            if i is None or errors:
                break
            j = free_y.get()
            final = pos + n == total
            y = renderer.render_pcm(xs[i][:, :n], yaw=tracks, final=final, ring_out=final and ring_out,
                                    out=ys[j][:, :n + (reach if final else 0)], out_bits=out_bits)
            free_x.put(i)
            full_y.put((j, pos, y.shape[1]))
    finally:
        free_x.put(None)
        full_y.put(None)
        for t in threads:
            t.join()
    if errors:
        raise errors[0]
    return written
