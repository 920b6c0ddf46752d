"""Integer PCM beside the session renderer: the codec on torch tensors of any device, and a RIFF reader of our own.

* `pcm_decode_device`, `pcm_encode_device`: the bits of session.pcm_decode / session.pcm_encode as a handful of torch copies and
  elementwise operations on tensors the caller provides -- SessionRenderer.render_pcm runs them on its compute stream in front of
  and behind the kernels, so that integer samples, not floats, cross the link.  Nothing is allocated per call.
* `WavReader`: the `fmt ` and `data` chunks of a PCM WAV, format tag 1 or WAVE_FORMAT_EXTENSIBLE with the integer-PCM sub-format
  (the header nearly every real 24-bit or multichannel file carries, which the stdlib `wave` of Python 3.10 refuses);
  `readinto` puts frames into the caller's array without a `bytes` in between.

Little-endian hosts only: an int32 word is viewed as its four bytes, the low one first.
"""
from __future__ import annotations

import struct
import sys

__all__ = ["PCM_BITS", "pcm_decode_device", "pcm_encode_device", "pcm_shape", "pcm_dtype", "WavReader"]

PCM_BITS = (16, 24, 32)

if sys.byteorder != "little":                   # pragma: no cover
    raise ImportError("open_headstage_amd.pcm views int32 words as little-endian bytes")


def pcm_dtype(lib, bits):
    """the sample dtype of `bits`-bit PCM in `lib` (numpy or torch): int16, int32, or uint8 for the packed 24-bit bytes"""
    return {16: lib.int16, 24: lib.uint8, 32: lib.int32}[bits]


def pcm_shape(bits, n_streams, frames, channels):
    """the shape of interleaved PCM in WAV frame order: [S][frames][C], 24-bit packed [S][frames][C][3] (uint8)"""
    return (n_streams, frames, channels, 3) if bits == 24 else (n_streams, frames, channels)


def _check(t, dtype, shape, what):
    if t is None or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = "None" if t is None else f"{t.dtype} {tuple(t.shape)}"
        raise ValueError(f"{what}: expected {dtype} {tuple(shape)}, got {got}")


def pcm_decode_device(raw, bits, out, word=None):
    """interleaved little-endian PCM raw [S][n][C] (int16 / int32; 24-bit: packed uint8 [S][n][C][3]) -> planar float32 out
    [S][C][n], value = int / 2^(bits - 1): the bits of session.pcm_decode.  Tensors of one device, any strides.

    16 / 32: one permuting, converting copy and a multiplication by a power of two; the only rounding is int32 -> float32 (to
    nearest even, as pcm_decode rounds its exact float64).  24: the three bytes go into bytes 1..3 of `word`, an int32 [S][n][C]
    scratch whose LOW BYTES ARE ZERO (torch.zeros once: this function writes the other three only, so they stay zero); the word
    is then value * 256, sign included, and is decoded as 32 bits -- 24 significant bits are exact in float32."""
    import torch
    if bits not in PCM_BITS:
        raise ValueError(f"PCM of {bits} bits: 16, 24 or 32 are read")
    if out.dtype != torch.float32 or out.ndim != 3:
        raise ValueError(f"out: expected float32 [S][C][n], got {out.dtype} {tuple(out.shape)}")
    S, C, n = out.shape
    _check(raw, pcm_dtype(torch, bits), pcm_shape(bits, S, n, C), "raw")
    if bits == 24:
        _check(word, torch.int32, (S, n, C), "word")
        if not word.is_contiguous():
            raise ValueError("word: a contiguous int32 scratch")
        word.view(torch.uint8).view(S, n, C, 4)[..., 1:].copy_(raw)
        raw = word
    out.copy_(raw.permute(0, 2, 1))
    out.mul_(2.0 ** -15 if bits == 16 else 2.0 ** -31)
    return out


def pcm_encode_device(y, bits, out, f64, word=None):
    """planar float32 y [S][2][n] -> interleaved little-endian PCM out [S][n][2] (int16 / int32; 24-bit: packed uint8
    [S][n][2][3]): y 2^(bits - 1), rounded half to even, clipped to [-2^(bits - 1), 2^(bits - 1) - 1], no dither -- the bits of
    session.pcm_encode for every finite input.  f64: float64 scratch [S][2][n]; the multiplication, the rounding and the clip run
    there, because 2^31 - 1 is no float32 and 1.0 must become 0x7FFFFFFF.  24: `word`, an int32 scratch [S][n][2], takes the
    integers; out gets their low three bytes."""
    import torch
    if bits not in PCM_BITS:
        raise ValueError(f"PCM of {bits} bits: 16, 24 or 32 are written")
    if y.dtype != torch.float32 or y.ndim != 3:
        raise ValueError(f"y: expected float32 [S][channels][n], got {y.dtype} {tuple(y.shape)}")
    S, C, n = y.shape
    _check(f64, torch.float64, (S, C, n), "f64")
    _check(out, pcm_dtype(torch, bits), pcm_shape(bits, S, n, C), "out")
    full = float(1 << (bits - 1))
    f64.copy_(y)
    f64.mul_(full)
    f64.round_()
    f64.clamp_(-full, full - 1.0)
    if bits != 24:
        out.copy_(f64.permute(0, 2, 1))
        return out
    _check(word, torch.int32, (S, n, C), "word")
    if not word.is_contiguous():
        raise ValueError("word: a contiguous int32 scratch")
    word.copy_(f64.permute(0, 2, 1))
    out.copy_(word.view(torch.uint8).view(S, n, C, 4)[..., :3])
    return out


# ---- RIFF ----------------------------------------------------------------------------------------------------------------------
_TAG_PCM, _TAG_EXTENSIBLE = 0x0001, 0xFFFE
_FMT_MAX = 256                                  # bytes of a fmt chunk that is still read (EXTENSIBLE has 40)
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")         # KSDATAFORMAT_SUBTYPE_*: the format tag, then these 14 bytes


class WavReader:
    """The frames of an integer PCM WAV.  `.channels`, `.bits` (16 / 24 / 32), `.rate`, `.frames`, `.frame_bytes`; readinto() and
    readframes() walk the `data` chunk from its start.  Accepts format tag 1 and WAVE_FORMAT_EXTENSIBLE with the PCM sub-format
    whose valid bits equal the container's; every other file is a ValueError (float, compressed, 8-bit, fewer valid bits than the
    container holds, no `data` chunk, a header that ends early).  Chunks other than `fmt ` and `data` are skipped, pad byte
    included; RF64 is not read."""

    def __init__(self, path):
        self._f = open(path, "rb")
        try:
            self._parse(str(path))
        except BaseException:
            self._f.close()
            raise

    def _need(self, n, path, what):
        b = self._f.read(n)
        if len(b) != n:
            raise ValueError(f"{path}: the file ends inside {what}")
        return b

    def _parse(self, path):
        f = self._f
        head = f.read(12)
        if len(head) != 12 or head[:4] != b"RIFF" or head[8:] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = None
        while True:
            h = f.read(8)
            if not h:
                raise ValueError(f"{path}: no data chunk")
            if len(h) != 8:
                raise ValueError(f"{path}: the file ends inside a chunk header")
            cid, size = h[:4], struct.unpack("<I", h[4:])[0]
            if cid == b"fmt ":
                if not 16 <= size <= _FMT_MAX:
                    raise ValueError(f"{path}: a fmt chunk of {size} bytes")
                fmt = self._need(size, path, "the fmt chunk")
                if size & 1:
                    f.seek(1, 1)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: the data chunk comes before the fmt chunk")
                break
            else:
                f.seek(size + (size & 1), 1)
        tag, ch, rate, _, align, bits = struct.unpack("<HHIIHH", fmt[:16])
        if tag == _TAG_EXTENSIBLE:
            if len(fmt) < 40 or struct.unpack("<H", fmt[16:18])[0] < 22:
                raise ValueError(f"{path}: a WAVE_FORMAT_EXTENSIBLE header that is too short")
            valid, sub = struct.unpack("<H", fmt[18:20])[0], fmt[24:40]
            if sub[2:] != _GUID_TAIL or struct.unpack("<H", sub[:2])[0] != _TAG_PCM:
                raise ValueError(f"{path}: the sub-format is not integer PCM")
            if valid != bits:
                raise ValueError(f"{path}: {valid} valid bits in a {bits}-bit container")
        elif tag != _TAG_PCM:
            raise ValueError(f"{path}: format tag {tag:#x}, integer PCM (1 or 0xFFFE) is read")
        if bits not in PCM_BITS:
            raise ValueError(f"{path}: {bits}-bit samples; 16, 24 or 32-bit integer PCM only")
        if ch < 1 or rate < 1 or align != ch * bits // 8:
            raise ValueError(f"{path}: {ch} channels of {bits} bits at {rate} Hz in frames of {align} bytes")
        self.channels, self.bits, self.rate, self.frame_bytes = ch, bits, rate, align
        start = f.tell()
        end = f.seek(0, 2)
        f.seek(start)
        self.frames = min(size, end - start) // align            # (a data chunk cut short holds the frames that are there)
        self._left = self.frames

    def readinto(self, buffer, frames):
        """the next min(frames, what is left) frames into the front of `buffer` (anything C-contiguous and writable: a slice of
        the call's array) -> frames read"""
        k = max(0, min(int(frames), self._left))
        if k == 0:
            return 0
        mv = memoryview(buffer).cast("B")
        nbytes = k * self.frame_bytes
        if nbytes > len(mv):
            raise ValueError(f"{k} frames need {nbytes} bytes, the buffer holds {len(mv)}")
        got = 0
        while got < nbytes:
            m = self._f.readinto(mv[got:nbytes])
            if not m:
                raise ValueError("the file ended inside its data chunk")
            got += m
        self._left -= k
        return k

    def readframes(self, frames) -> bytes:
        b = bytearray(max(0, min(int(frames), self._left)) * self.frame_bytes)
        self.readinto(b, frames)
        return bytes(b)

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
