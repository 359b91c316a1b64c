"""Host-side mirror of the reference's interface for the hot path, on top of libsdrhip.so.

Class and method names follow the reference (Decimators.h:32-71, Interpolators.h:35-61,
Downsampler.h:26-83, Upsampler.h:27-70, the CM256 call sites UDPSinkFEC.cpp:195-246 /
SDRdaemonFECBuffer.cpp:148-213) so that the parity tests read like code written against the
reference.  Every method accepts

  * numpy int16 arrays  -> SDRHIP_MEM_HOST (staged through the GPU, synchronous), or
  * torch int16 CUDA tensors -> SDRHIP_MEM_DEVICE (zero-copy, enqueued on the context stream).

The Rx / Tx pipes also take / give 8-bit IQ (RxPipe input_format "u8" = RTL-SDR offset binary as uint8, "s8" = HackRF int8;
TxPipe output_format "s8" = HackRF int8), with the same shapes.

Shapes: one stream (n, 2); a bank of S streams (S, n, 2).  There is no CPU implementation
behind these classes: without libsdrhip.so or without a GPU they raise.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (BLOCK_BYTES, DGRAM_SKIP, FC_CEN, FC_INF, FC_SUP, HB_DB, HB_EO1, MEM_DEVICE, MEM_HOST, NB_ORIGINAL,  # noqa: F401
                   SAMPLES_PER_FRAME, UDPSIZE, CM256Block, CM256Params, RxConfig, SdrHipError, check)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


K_DECIMATE, K_INTERPOLATE, K_FEC_ENCODE, K_FEC_DECODE, K_CONVERT = 0, 1, 2, 3, 4

# IQ sample formats (SDRHIP_IQ_*): code and element dtype
_IQ_FORMATS = {"s16": (0, np.int16), "u8": (1, np.uint8), "s8": (2, np.int8)}


def _iq_format(fmt, allowed):
    if fmt not in allowed:
        raise ValueError("IQ format must be one of %s, not %r" % (", ".join(allowed), fmt))
    return _IQ_FORMATS[fmt]


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def device_count():
    return _lib.lib().sdrhip_device_count()


class _Handle:
    """A library handle its object owns: self.h, given back once by close() -- the class's `_destroy` entry -- at the latest
    when the object dies."""

    _destroy = None

    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()

    def close(self):
        if getattr(self, "h", None):  # (an object whose constructor raised early has none)
            getattr(self.lib, self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One per GPU (sdrhip_ctx).  stream: a torch.cuda.Stream, a raw hipStream_t int, or None
    (torch's current stream when torch sees the device, else the null stream)."""

    _destroy = "sdrhip_ctx_destroy"

    def __init__(self, device=0, stream=None):
        _Handle.__init__(self, _lib.lib())
        self.device = device
        if stream is None and torch is not None and torch.cuda.is_available():
            with torch.cuda.device(device):
                stream = torch.cuda.current_stream().cuda_stream
        elif stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self.options = {}
        self._host_allocs = {}  # address of every host_alloc array -> the pointer to free
        check(self.lib.sdrhip_ctx_create(device, C.c_void_p(stream or 0), C.byref(self.h)))

    def synchronize(self):
        check(self.lib.sdrhip_ctx_synchronize(self.h))

    def set_option(self, key, value):
        """kernel-path knobs for tests and tools (sdrhip_ctx_set_option): decim_path, mfma_span, mfma_min, interp_path,
        interp_span, rx_fused; the defaults were read from the SDRHIP_* environment when the context was created.
        "dec_max_rows" = 1..128 is a promise about the sender's fecblk (it bounds the recovery blocks' row indices, not only their
        count); "auto" is no promise: the batched decoder decides per frame from its block indices -- at most 32 recovery blocks, all
        of rows 0..31: repaired in the one launch that plans it; any other frame is deferred to the general chain behind that launch
        -- and delivers the bytes of dec_max_rows = 128"""
        check(self.lib.sdrhip_ctx_set_option(self.h, str(key).encode(), str(value).encode()))
        self.options[str(key)] = str(value)

    def option(self, key, default=None):
        """what this Context was last TOLD for `key`: by set_option, else by the SDRHIP_<KEY> environment variable that the library
        read when the context was created, else `default` (the library's own default is not queried)"""
        if key in self.options:
            return self.options[key]
        return os.environ.get("SDRHIP_" + str(key).upper(), default)

    def host_alloc(self, shape, dtype=np.int16):
        """numpy array on pinned host memory of the library (sdrhip_host_alloc): blocks submitted from it are uploaded in
        place.  Keep the Context alive while the array is in use; free with host_free(array)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.sdrhip_host_alloc(self.h, n)
        if not p:
            raise MemoryError("sdrhip_host_alloc(%d) failed" % n)
        buf = (C.c_char * n).from_address(p)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._host_allocs[a.ctypes.data] = p
        return a

    def host_free(self, a):
        p = self._host_allocs.pop(a.ctypes.data, None)
        if p:
            self.lib.sdrhip_host_free(self.h, C.c_void_p(p))

    def counter(self, key):
        """event counters (sdrhip_ctx_get_counter): "dec_rows_exceeded" = frames the batched decoder left unrepaired because they
        carried more recovery blocks than the dec_max_rows option promises (device-side: synchronises; does not grow under
        dec_max_rows = auto); "dec_deferred" = frames the one-launch decoder deferred under dec_max_rows = auto (device-side); "h2d_bytes" / "d2h_bytes" =
        bytes the context's calls copied across the host link since it was created (host-side: no synchronisation)"""
        v = C.c_uint64(0)
        check(self.lib.sdrhip_ctx_get_counter(self.h, str(key).encode(), C.byref(v)))
        return v.value

    def timing_begin(self):
        check(self.lib.sdrhip_ctx_timing_begin(self.h))

    def timing_end(self):
        ms = C.c_float(0)
        check(self.lib.sdrhip_ctx_timing_end(self.h, C.byref(ms)))
        return ms.value

    def kernel_timing(self, enable=True):
        check(self.lib.sdrhip_ctx_kernel_timing(self.h, 1 if enable else 0))

    def kernel_timing_read(self, kernel_class):
        """-> (total_ms, launches) of the kernel class since the last read (K_* constants)"""
        ms, n = C.c_double(0), C.c_uint(0)
        check(self.lib.sdrhip_ctx_kernel_timing_read(self.h, kernel_class, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _bank_view(iq, nstreams, dtype=np.int16):
    """-> (array (S, n, 2) contiguous-per-stream, is_torch, squeeze).  dtype: the element type the call takes (np.int16, or for
    8-bit IQ np.uint8 / np.int8, which may also come flat interleaved: (2n,) or (S, 2n))"""
    squeeze = False
    eight = dtype != np.int16
    if _is_torch(iq):
        tdt = {np.int16: torch.int16, np.uint8: torch.uint8, np.int8: torch.int8}[dtype]
        if iq.dtype != tdt or not iq.is_cuda:
            raise TypeError("torch input must be a %s CUDA tensor" % str(tdt).replace("torch.", ""))
        if eight and iq.dim() == 1:
            iq = iq.reshape(-1, 2)
        elif eight and iq.dim() == 2 and iq.shape[1] != 2:
            iq = iq.reshape(iq.shape[0], -1, 2)
        if iq.dim() == 2:
            iq, squeeze = iq.unsqueeze(0), True
        if iq.dim() != 3 or iq.shape[2] != 2 or iq.shape[0] != nstreams:
            raise ValueError("expected shape (%d, n, 2)" % nstreams)
        if iq.stride(2) != 1 or iq.stride(1) != 2:
            iq = iq.contiguous()
        return iq, True, squeeze
    a = np.asarray(iq)
    if a.dtype != dtype:
        raise TypeError("numpy input must be %s" % np.dtype(dtype).name)
    if eight and a.ndim == 1:
        a = a.reshape(-1, 2)
    elif eight and a.ndim == 2 and a.shape[1] != 2:
        a = a.reshape(a.shape[0], -1, 2)
    if a.ndim == 2:
        a, squeeze = a[None], True
    if a.ndim != 3 or a.shape[2] != 2 or a.shape[0] != nstreams:
        raise ValueError("expected shape (%d, n, 2)" % nstreams)
    return np.ascontiguousarray(a), False, squeeze


def _ptr(x):
    return C.c_void_p(x.data_ptr()) if _is_torch(x) else C.c_void_p(x.ctypes.data)


def _stride_samples(x):
    return (x.stride(0) // 2) if _is_torch(x) else (x.strides[0] // (2 * x.itemsize))


def _padded_rows(S, n, m, dtype, device, src=None, zero=False):
    """torch rows (S, n, 2) of a buffer whose rows are a multiple of m samples long (and not empty): the library's stride rule
    for device banks, 16-byte aligned rows.  src: a tensor (S, n, 2) copied into them."""
    buf = (torch.zeros if zero else torch.empty)((S, max((n + m - 1) & ~(m - 1), m), 2), dtype=dtype, device=device)
    if src is not None:
        buf[:, :n].copy_(src)
    return buf[:, :n]


def _rows_in_place(a, S, dtype):
    """whether the rows of a host array are usable where they lie, with their stride: (S, n, 2) of dtype, samples contiguous, the
    rows a whole number of samples apart (rows of a bigger array, e.g. a pinned buffer)"""
    it = np.dtype(dtype).itemsize
    return (a.ndim == 3 and a.dtype == dtype and a.shape[0] == S and a.shape[2] == 2 and a.strides[2] == it
            and a.strides[1] == 2 * it and a.strides[0] % (2 * it) == 0 and a.strides[0] > 0)


def _stamps(v, S):
    """a time stamp field -- a scalar, None (= 0) or one value per stream -- as the (C.c_uint32 * S) the per-stream entries take"""
    v = np.broadcast_to(np.asarray(0 if v is None else v, dtype=np.uint32), (S,))
    return (C.c_uint32 * S)(*[int(x) for x in v])


def _frame_buffer(S, cap, nb_fec, device=None, out=None):
    """-> (the frame output buffer (S, cap, 128 + nb_fec, 512) uint8 -- torch on `device`, numpy without one, or the caller's
    `out` if it has the room --, its stride in bytes per stream)"""
    rows = NB_ORIGINAL + nb_fec
    if out is None:
        shape = (S, cap, rows, UDPSIZE)
        out = torch.empty(shape, dtype=torch.uint8, device=device) if device is not None else np.empty(shape, np.uint8)
    if out.shape[1] < cap or out.shape[0] != S:
        raise ValueError("out must hold (S, >= %d, %d, 512) bytes" % (cap, rows))
    return out, out.shape[1] * rows * UDPSIZE


def _records(info, F, n):
    """the sdrhip_fecbuf_frame records a call filled in, F slots per stream (info may be None when every n[s] is 0): per stream
    the list of dicts of its first n[s]"""
    return [[dict(frame_index=r.frame_index, block_count=r.block_count, recovery_count=r.recovery_count, flags=r.flags)
             for r in (info[s * F:s * F + int(n[s])] if n[s] else ())] for s in range(len(n))]


def _packed_datagrams(dgrams_per_stream, S):
    """what the submit_datagrams methods take -- one (n_s, 512) uint8 host array per stream, or (array, counts) of them back to
    back -- as (packed contiguous uint8 array, used where it lies when it is one already; counts)"""
    if isinstance(dgrams_per_stream, tuple):
        buf, counts = dgrams_per_stream
        counts = [int(x) for x in counts]
        if len(counts) != S:
            raise ValueError("one count per stream")
    else:
        if len(dgrams_per_stream) != S:
            raise ValueError("one datagram array per stream")
        if any(_is_torch(d) for d in dgrams_per_stream):
            raise TypeError("submit_datagrams takes host memory")
        counts = [int(np.asarray(d).shape[0]) for d in dgrams_per_stream]
        nz = [np.asarray(d, np.uint8).reshape(-1, UDPSIZE) for d in dgrams_per_stream if len(d)]
        buf = np.concatenate(nz) if nz else np.zeros((0, UDPSIZE), np.uint8)
    if _is_torch(buf):
        raise TypeError("submit_datagrams takes host memory")
    buf = np.ascontiguousarray(buf, np.uint8)
    if buf.size != sum(counts) * UDPSIZE:
        raise ValueError("the datagrams do not match the counts")
    return buf, counts


class _BatchLog:
    """What a pipe knows about the batches its library handle holds (the asynchronous entries): the batches launched and not
    collected yet, oldest first, and the one still being filled.  Pure bookkeeping: collects size and shape their buffers from
    the head record, since a batch in flight keeps the configuration it was launched with.  A record has
      kind  "uniform" | "ragged" | "datagram" (Rx), "frames" | "datagram" (Tx)
      size  the hint the collects size with: samples per stream, per-stream counts (numpy), frames; None for datagrams
      cfg   the setting the batch keeps: nb_fec (Rx), log2interp (Tx), as it stood when the batch was launched
    A fresh log is the library's default ring: 4 batches of one block."""

    class Batch:
        def __init__(self, kind, size, cfg=None):
            self.kind, self.size, self.cfg, self.nblocks = kind, size, cfg, 1

        @property
        def most(self):
            """the largest count of a stream (0 for a size of None)"""
            if isinstance(self.size, np.ndarray):
                return int(self.size.max()) if self.size.size else 0
            return self.size or 0

    def __init__(self, blocks=1):
        self.reset(blocks)

    def reset(self, blocks=1):
        """set_async: an empty ring whose batches take `blocks` submitted blocks each"""
        self.blocks, self.batches, self.filling = blocks, [], None
        self.last = 0  # size of the uniform batch collected last: a pipelined pipe delivers the PREVIOUS batch's frames

    def block(self, kind, size, cfg):
        """after a successful submit of one block of `size`: it joins the batch being filled, which the library launches -- under
        the cfg of this submit -- once it has `blocks` blocks"""
        if self.filling is None:
            self.filling = self.Batch(kind, size)
        else:
            self.filling.size = self.filling.size + size
            self.filling.nblocks += 1
        if self.filling.nblocks >= self.blocks:
            self._launch(cfg)

    def batch(self, kind, size, cfg):
        """after a successful submit that is a batch of its own, launched at once (datagram batches, Tx frames)"""
        self.batches.append(self.Batch(kind, size, cfg))

    def _launch(self, cfg):
        b, self.filling = self.filling, None
        b.cfg = cfg
        self.batches.append(b)

    def head(self, cfg, wait_kind=None):
        """-> (the record of the oldest launched batch or None, the cfg that batch keeps), for a collect; cfg: the pipe's setting
        at this moment, assumed for a batch the log was not told of.  wait_kind: the kind a collect with wait = True takes: with
        nothing in front of it the library sends the partly filled batch of that kind out as it is, under the cfg of this moment"""
        if not self.batches and self.filling is not None and self.filling.kind == wait_kind:
            self._launch(cfg)
        rec = self.batches[0] if self.batches else None
        return rec, (rec.cfg if rec is not None else cfg)

    def pop(self):
        """the oldest batch was collected (rc 0: not the -1 of a call that learns the counts, not SDRHIP_EBUSY).  A log that was
        not told of a submit (a caller of the C entry itself) has nothing to forget."""
        if self.batches:
            b = self.batches.pop(0)
            if b.kind == "uniform":
                self.last = b.size

    def sample_room(self):
        """samples per stream that bound what the next collect can deliver: the oldest batch, the one being filled, or -- a
        pipelined pipe -- the uniform batch collected last"""
        return max([self.last] + [b.most for b in (self.filling, self.batches[0] if self.batches else None) if b is not None])


def _counts(counts, S, n):
    """per-stream sample counts of a ragged call as a numpy int64 vector, each <= the rows' length n"""
    cnt = np.asarray(counts.cpu() if _is_torch(counts) else counts, dtype=np.int64).reshape(-1)
    if cnt.shape[0] != S or (S and (cnt.min() < 0 or cnt.max() > n)):
        raise ValueError("counts: %d values in 0..%d expected" % (S, n))
    return cnt


def _stream_mask(streams, S):
    """the mask argument of the sdrhip_*_reset_streams entries: None = NULL (every stream), else one byte per stream"""
    if streams is None:
        return None
    m = (C.c_uint8 * S)()
    for s in streams:
        s = int(s)
        if not 0 <= s < S:
            raise ValueError("stream %d of %d" % (s, S))
        m[s] = 1
    return m


def _export_stream(ctx, kind, h, stream):
    n = getattr(ctx.lib, "sdrhip_%s_stream_state_bytes" % kind)(h)
    buf = C.create_string_buffer(n)
    check(getattr(ctx.lib, "sdrhip_%s_export_stream" % kind)(h, int(stream), buf, n))
    return buf.raw


def _import_stream(ctx, kind, h, stream, blob):
    blob = bytes(blob)
    check(getattr(ctx.lib, "sdrhip_%s_import_stream" % kind)(h, int(stream), blob, len(blob)))


def _plan_dict(fn, h):
    p = _lib.DecimPlan()
    check(fn(h, C.byref(p)))
    return {"path": {0: None, 1: "valu", 2: "mfma"}[p.path], "span": p.span, "wps": p.wps, "npieces": p.npieces, "nseg": p.nseg,
            "head": p.head, "tail_start": p.tail_start}


class Decimators(_Handle):
    """Bank of reference `Decimators` objects (Decimators.h:32-71)."""

    _destroy = "sdrhip_decimators_destroy"

    def __init__(self, ctx, nstreams=1, hb_variant=HB_EO1):
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams = ctx, nstreams
        check(ctx.lib.sdrhip_decimators_create(ctx.h, nstreams, hb_variant, C.byref(self.h)))

    def reset(self, streams=None):
        """constructor state: every stream (sdrhip_decimators_reset), or the streams listed (sdrhip_decimators_reset_streams:
        on the device, no synchronisation, the others run on)"""
        if streams is None:
            check(self.ctx.lib.sdrhip_decimators_reset(self.h))
        else:
            check(self.ctx.lib.sdrhip_decimators_reset_streams(self.h, _stream_mask(streams, self.nstreams)))

    def decimate(self, log2decim, fcpos, sample_size, iq, out=None):
        """Decimators::decimate<2^log2decim>_{inf,sup,cen}(sampleSize, in, out).
        Returns (out, new_sample_size)."""
        x, is_t, squeeze = _bank_view(iq, self.nstreams)
        S, n = x.shape[0], x.shape[1]
        n_res = (n >> log2decim) if 0 <= log2decim <= 6 else 0  # out-of-range factors are rejected by the library
        if out is None:
            out = _padded_rows(S, n_res, 4, torch.int16, x.device) if is_t else np.empty((S, n_res, 2), dtype=np.int16)
        if is_t and S > 1 and (x.stride(0) // 2) % 4:
            raise ValueError("device bank input: per-stream stride must be a multiple of 4 samples")
        ss = C.c_uint(sample_size)
        n_out = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_decimate(self.h, log2decim, fcpos, C.byref(ss), _ptr(x), n, _stride_samples(x), _ptr(out),
                                           _stride_samples(out) if S > 1 else n_res, C.byref(n_out),
                                           MEM_DEVICE if is_t else MEM_HOST))
        return (out[0] if squeeze else out), ss.value

    def decimate_ragged(self, log2decim, fcpos, sample_size, iq, counts, out=None):
        """sdrhip_decimate_ragged: stream s decimates counts[s] samples of row s of iq (S, >= max(counts), 2).
        Returns (out (S, max(counts) >> log2decim, 2) -- row s valid up to n_out[s] --, n_out (numpy, S), new_sample_size).
        sample_size: one size for the bank, or a sequence of one size per stream (sdrhip_decimate_ragged_bits: stream s is
        shifted for its own size); new_sample_size then is the list of the streams' new sizes."""
        x, is_t, _ = _bank_view(iq, self.nstreams)
        S, n = x.shape[0], x.shape[1]
        cnt = _counts(counts, S, n)
        mx = int(cnt.max()) if S else 0
        n_res = (mx >> log2decim) if 0 <= log2decim <= 6 else 0
        if out is None:
            out = _padded_rows(S, n_res, 4, torch.int16, x.device, zero=True) if is_t else np.zeros((S, n_res, 2), dtype=np.int16)
        if is_t and S > 1 and (x.stride(0) // 2) % 4:
            raise ValueError("device bank input: per-stream stride must be a multiple of 4 samples")
        n_out = (C.c_size_t * S)()
        per_stream = not isinstance(sample_size, (int, np.integer))
        if per_stream:
            sizes = [int(b) for b in sample_size]
            if len(sizes) != S:
                raise ValueError("sample_size: %d sizes, one per stream" % S)
            ss = (C.c_uint * S)(*sizes)
            entry, ssp = self.ctx.lib.sdrhip_decimate_ragged_bits, ss
        else:
            ss = C.c_uint(sample_size)
            entry, ssp = self.ctx.lib.sdrhip_decimate_ragged, C.byref(ss)
        check(entry(self.h, log2decim, fcpos, ssp, _ptr(x), (C.c_size_t * S)(*cnt.tolist()), _stride_samples(x), _ptr(out),
                    _stride_samples(out) if S > 1 else n_res, n_out, MEM_DEVICE if is_t else MEM_HOST))
        return out, np.array(n_out[:], dtype=np.int64), (list(ss) if per_stream else ss.value)

    def decimate_taps(self, taps, sample_size, iq, counts=None, out=None):
        """sdrhip_decimate_taps: every rate of a centred cascade in one launch.  taps: the log2 decimations wanted (1..6); stream s
        consumes counts[s] samples of row s of iq (S, >= max(counts), 2), None: the full rows; numpy or a device tensor, as
        decimate_ragged.  Returns ({k: out_k (S, max(n_used) >> k, 2) -- row s valid up to n_used[s] >> k --}, {k: sample size
        after decimate<2^k>_cen}, n_used (numpy, S)): what Decimators::decimate<2^k>_cen gives on x[:n_used[s]], for every k, and
        the bank left as by decimate_ragged(max(taps), FC_CEN, ...).  out: {k: buffer} to write into."""
        x, is_t, _ = _bank_view(iq, self.nstreams)
        S, n = x.shape[0], x.shape[1]
        cnt = _counts([n] * S if counts is None else counts, S, n)
        ks = sorted(set(int(k) for k in taps))
        if any(not 0 <= k < 32 for k in ks):
            raise ValueError("taps: log2 decimations expected")
        mask = sum(1 << k for k in ks)
        ok = bool(ks) and not mask & ~0x7e  # (anything else: the library refuses the mask; no buffers are needed for that)
        L = ks[-1] if ok else 0
        mx = ((int(cnt.max()) if S else 0) >> L) << L
        if is_t and S > 1 and (x.stride(0) // 2) % 4:
            raise ValueError("device bank input: per-stream stride must be a multiple of 4 samples")
        t = _lib.DecimTaps()
        outs = {}
        for k in (ks if ok else ()):
            o = None if out is None else out.get(k)
            if o is None:
                o = _padded_rows(S, mx >> k, 4, torch.int16, x.device, zero=True) if is_t else np.zeros((S, mx >> k, 2), dtype=np.int16)
            outs[k] = o
            t.iq_out[k] = _ptr(o).value
            t.out_stride[k] = _stride_samples(o) if S > 1 else mx >> k
        n_used = (C.c_size_t * S)()
        check(self.ctx.lib.sdrhip_decimate_taps(self.h, mask, sample_size, _ptr(x), (C.c_size_t * S)(*cnt.tolist()), _stride_samples(x),
                                                C.byref(t), n_used, MEM_DEVICE if is_t else MEM_HOST))
        return outs, {k: int(t.sample_size[k]) for k in outs}, np.array(n_used[:], dtype=np.int64)

    def last_plan(self):
        """what the last cascade launch was (sdrhip_decimators_last_plan): dict with path ('valu' / 'mfma' / None), span, wps, ..."""
        return _plan_dict(self.ctx.lib.sdrhip_decimators_last_plan, self.h)


class Downsampler:
    """Reference `Downsampler` (Downsampler.h:26-83): configuration + dispatch."""

    def __init__(self, ctx, decim=0, fcpos=FC_CEN, nstreams=1, hb_variant=HB_EO1):
        self.m_decim, self.m_fcPos = decim, fcpos
        self.m_error = ""
        self.m_decimators = Decimators(ctx, nstreams, hb_variant)

    def configure(self, m):
        """m: dict of the parsekv pairs (Downsampler.cpp:32-67).  Returns False and sets error()
        on an invalid value, like the reference."""
        if "decim" in m:
            v = int(m["decim"])
            if v < 0 or v > 6:
                self.m_error = "Invalid log2 decimation factor"
                return False
            self.m_decim = v
        if "fcpos" in m:
            v = int(m["fcpos"])
            if v < FC_INF or v > FC_CEN:
                self.m_error = "Invalid Fc position index"
                return False
            self.m_fcPos = v
        return True

    def getLog2Decimation(self):
        return self.m_decim

    def error(self):
        e, self.m_error = self.m_error, ""
        return e

    def __bool__(self):
        return not self.m_error

    def process(self, sample_size, samples_in):
        """Downsampler::process (Downsampler.cpp:74-162) -> (samples_out, sampleSize)."""
        return self.m_decimators.decimate(self.m_decim, self.m_fcPos, sample_size, samples_in)

    def rescale(self, sample_size, samples_inout):
        """Downsampler::rescale = Decimators::decimate1 (Downsampler.cpp:69-72)."""
        return self.m_decimators.decimate(0, self.m_fcPos, sample_size, samples_inout)


class TestSource(_Handle):
    """Bank of the reference's TestSource devices (TestSource.h:29-116) generating on the GPU: configure() takes the
    reference's control string / key-value map (TestSource.cpp:59-215), read() returns the next samples of every
    stream as a CUDA tensor (or numpy with host=True).  The sample arithmetic is the library's integer NCO."""

    _destroy = "sdrhip_testsource_destroy"

    def __init__(self, ctx, nstreams=1):
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams = ctx, nstreams
        self.m_error = ""
        check(ctx.lib.sdrhip_testsource_create(ctx.h, nstreams, C.byref(self.h)))

    def configure(self, m, stream=-1):
        """-> bool like TestSource::configure; the message is kept for error()"""
        kv = m if isinstance(m, str) else ",".join("%s=%s" % (k, v) for k, v in m.items())
        try:
            check(self.ctx.lib.sdrhip_testsource_configure(self.h, stream, kv.encode()))
        except SdrHipError as e:
            self.m_error = str(e)
            return False
        return True

    def error(self):
        e, self.m_error = self.m_error, ""
        return e

    def get(self, stream=0):
        sr, fr, bl, dc, fc = C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.ctx.lib.sdrhip_testsource_get(self.h, stream, C.byref(sr), C.byref(fr), C.byref(bl), C.byref(dc), C.byref(fc)))
        return {"sample_rate": sr.value, "frequency": fr.value, "block_length": bl.value, "decim": dc.value, "fcpos": fc.value}

    def get_sample_rate(self, stream=0):
        return self.get(stream)["sample_rate"]

    def get_frequency(self, stream=0):
        return self.get(stream)["frequency"]

    def read(self, n, host=False, out=None):
        """-> (S, n, 2) int16 (squeezed for one stream)"""
        S = self.nstreams
        pad = (n + 3) & ~3
        if out is None:
            out = np.empty((S, pad, 2), np.int16) if host else torch.empty((S, pad, 2), dtype=torch.int16, device=torch.device("cuda", self.ctx.device))
        check(self.ctx.lib.sdrhip_testsource_read(self.h, _ptr(out), n, out.shape[1], MEM_HOST if host else MEM_DEVICE))
        y = out[:, :n]
        return y[0] if S == 1 else y


class Interpolators(_Handle):
    """Bank of reference `Interpolators` objects (Interpolators.h:35-61)."""

    _destroy = "sdrhip_interpolators_destroy"

    def __init__(self, ctx, nstreams=1):
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams = ctx, nstreams
        check(ctx.lib.sdrhip_interpolators_create(ctx.h, nstreams, C.byref(self.h)))

    def reset(self, streams=None):
        """constructor state: every stream (sdrhip_interpolators_reset), or the streams listed (sdrhip_interpolators_reset_streams)"""
        if streams is None:
            check(self.ctx.lib.sdrhip_interpolators_reset(self.h))
        else:
            check(self.ctx.lib.sdrhip_interpolators_reset_streams(self.h, _stream_mask(streams, self.nstreams)))

    def interpolate(self, log2interp, iq, out=None):
        """Interpolators::interpolate<2^log2interp>_cen(in, out)."""
        x, is_t, squeeze = _bank_view(iq, self.nstreams)
        S, n = x.shape[0], x.shape[1]
        n_res = (n << log2interp) if 0 <= log2interp <= 6 else 0
        if out is None:
            out = _padded_rows(S, n_res, 4, torch.int16, x.device) if is_t else np.empty((S, n_res, 2), dtype=np.int16)
        n_out = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_interpolate(self.h, log2interp, _ptr(x), n, _stride_samples(x), _ptr(out),
                                              _stride_samples(out) if S > 1 else n_res, C.byref(n_out),
                                              MEM_DEVICE if is_t else MEM_HOST))
        return out[0] if squeeze else out

    def interpolate_ragged(self, log2interp, iq, counts, out=None):
        """sdrhip_interpolate_ragged: stream s interpolates counts[s] samples of row s of iq (S, >= max(counts), 2) in one launch
        on a compact grid.  Returns (out (S, max(counts) << log2interp, 2) -- row s valid up to n_out[s] --, n_out (numpy, S))."""
        x, is_t, _ = _bank_view(iq, self.nstreams)
        S, n = x.shape[0], x.shape[1]
        cnt = _counts(counts, S, n)
        mx = int(cnt.max()) if S else 0
        n_res = (mx << log2interp) if 0 <= log2interp <= 6 else 0
        if out is None:
            out = _padded_rows(S, n_res, 4, torch.int16, x.device, zero=True) if is_t else np.zeros((S, n_res, 2), dtype=np.int16)
        if is_t and S > 1 and (x.stride(0) // 2) % 4:
            raise ValueError("device bank input: per-stream stride must be a multiple of 4 samples")
        n_out = (C.c_size_t * S)()
        check(self.ctx.lib.sdrhip_interpolate_ragged(self.h, log2interp, _ptr(x), (C.c_size_t * S)(*cnt.tolist()), _stride_samples(x), _ptr(out),
                                                     _stride_samples(out) if S > 1 else n_res, n_out, MEM_DEVICE if is_t else MEM_HOST))
        return out, np.array(n_out[:], dtype=np.int64)

    def last_plan(self):
        """what the last launch was (sdrhip_interpolators_last_plan): dict with path ('copy' / 'valu' / 'wave' / None), seg_len in
        inputs, wpw, entries = the (stream, segment) pairs served, compact = whether the grid was the ragged entry's"""
        p = _lib.InterpPlan()
        check(self.ctx.lib.sdrhip_interpolators_last_plan(self.h, C.byref(p)))
        return {"path": {0: None, 1: "copy", 2: "valu", 3: "wave"}[p.path], "seg_len": p.seg_len, "wpw": p.wpw, "entries": p.entries,
                "compact": bool(p.compact)}


class Upsampler:
    """Reference `Upsampler` (Upsampler.h:27-70)."""

    def __init__(self, ctx, interp=0, nstreams=1):
        self.m_interp = interp
        self.m_error = ""
        self.m_interpolators = Interpolators(ctx, nstreams)

    def configure(self, m):
        if "interp" in m:
            v = int(m["interp"])
            if v < 0 or v > 6:
                self.m_error = "Invalid log2 interpolation factor"
                return False
            self.m_interp = v
        return True

    def getLog2Interpolation(self):
        return self.m_interp

    def error(self):
        e, self.m_error = self.m_error, ""
        return e

    def process(self, samples_in):
        return self.m_interpolators.interpolate(self.m_interp, samples_in)


class CM256:
    """The `CM256` object of the reference's call sites (UDPSinkFEC.h:123, SDRdaemonFECBuffer.h:173)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def isInitialized(self):
        return True

    def cm256_encode(self, params, originals, recovery_out=None):
        """originals: (k, BlockBytes) uint8 numpy (taken positionally).  Returns (rc, recovery)."""
        k, m, bb = params
        originals = np.ascontiguousarray(originals, dtype=np.uint8)
        blocks = (CM256Block * k)()
        for i in range(k):
            blocks[i].Block = originals[i].ctypes.data
            blocks[i].Index = i
        rec = np.zeros((m, bb), dtype=np.uint8) if recovery_out is None else recovery_out
        rc = self.ctx.lib.sdrhip_cm256_encode(self.ctx.h, CM256Params(k, m, bb), blocks, C.c_void_p(rec.ctypes.data))
        return rc, rec

    def cm256_decode(self, params, data, indices):
        """data: (k, BlockBytes) uint8 received blocks, modified in place; indices: their Index
        fields.  Returns (rc, indices_after) -- the library's in-place contract."""
        k, m, bb = params
        assert data.dtype == np.uint8 and data.flags.c_contiguous and data.shape == (k, bb)
        blocks = (CM256Block * k)()
        for i in range(k):
            blocks[i].Block = data[i].ctypes.data
            blocks[i].Index = int(indices[i])
        rc = self.ctx.lib.sdrhip_cm256_decode(self.ctx.h, CM256Params(k, m, bb), blocks)
        return rc, np.array([blocks[i].Index for i in range(k)], dtype=np.uint8)


def fec_encode_frames(ctx, frames, nb_fec):
    """frames (F, 128, 512) uint8 (numpy or CUDA tensor) -> recovery super blocks (F, nb_fec, 512)."""
    is_t = _is_torch(frames)
    F = frames.shape[0]
    if not is_t:
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
    out = torch.zeros((F, nb_fec, 512), dtype=torch.uint8, device=frames.device) if is_t else np.zeros((F, nb_fec, 512), np.uint8)
    check(ctx.lib.sdrhip_fec_encode_frames(ctx.h, _ptr(frames), F, nb_fec, _ptr(out), MEM_DEVICE if is_t else MEM_HOST))
    return out


def fec_decode_frames(ctx, rx, indices=None, want_block0=False):
    """rx (F, 128, 512) uint8: first 128 received super blocks per frame, arrival order.
    -> payload (F, 127*508) uint8 [, block0 (F, 508)]"""
    is_t = _is_torch(rx)
    F = rx.shape[0]
    if not is_t:
        rx = np.ascontiguousarray(rx, dtype=np.uint8)
    if indices is not None:  # optional: by default the library reads header.blockIndex of the super blocks itself
        indices = np.ascontiguousarray(indices, dtype=np.uint8)
    if is_t:
        payload = torch.empty((F, 127 * 508), dtype=torch.uint8, device=rx.device)
        b0 = torch.empty((F, 508), dtype=torch.uint8, device=rx.device) if want_block0 else None
    else:
        payload = np.empty((F, 127 * 508), np.uint8)
        b0 = np.empty((F, 508), np.uint8) if want_block0 else None
    check(ctx.lib.sdrhip_fec_decode_frames(ctx.h, _ptr(rx), C.c_void_p(indices.ctypes.data if indices is not None else 0), F, _ptr(payload),
                                           _ptr(b0) if want_block0 else C.c_void_p(0), MEM_DEVICE if is_t else MEM_HOST))
    return (payload, b0) if want_block0 else payload


class _DeviceView:
    """A strided uint8 view of library-owned device memory (__cuda_array_interface__ v2)."""

    def __init__(self, ptr, shape, strides, device, owner=None):
        self.shape, self.device = tuple(shape), device
        self._owner = owner  # the handle whose memory this is: stays alive as long as the view (or a tensor made from it) does
        self.__cuda_array_interface__ = {"shape": tuple(shape), "strides": tuple(strides), "typestr": "|u1",
                                         "data": (ptr, False), "version": 2}

    def torch(self):
        """materialise as a torch tensor sharing the memory"""
        if self.shape[1] == 0:
            return torch.empty(self.shape, dtype=torch.uint8, device=self.device)
        return torch.as_tensor(self, device=self.device)


class RxPipe(_Handle):
    """Downsampler -> UDPSinkFEC framing -> CM256 encode for a bank of streams (sdrhip_rx)."""

    _destroy = "sdrhip_rx_destroy"

    def __init__(self, ctx, nstreams=1, log2decim=4, fcpos=FC_CEN, hb_variant=HB_EO1, sample_bits=16, nb_fec=32,
                 center_frequency_khz=435000, sample_rate=625000, pipelined=False, input_format="s16"):
        """pipelined: a process() call returns the frames the PREVIOUS call completed (their recovery blocks are computed inside
        this call's decimator launch, sdrhip_rx_set_pipelined); flush() / flush_view() return the last call's at the end.
        input_format: "s16" (int16 IQ), "u8" (RTL-SDR uint8 offset binary) or "s8" (HackRF int8), see set_input_format."""
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams, self.nb_fec = ctx, nstreams, nb_fec
        self._log = _BatchLog()  # the asynchronous batches in flight, each with the nb_fec it keeps (the collects size and shape with it)
        self.cfg = RxConfig(log2decim, fcpos, hb_variant, sample_bits, nb_fec, center_frequency_khz, sample_rate)
        self.m_error = ""
        self._stream_fec = None  # set_stream_fec's array (None: nb_fec is bank-wide)
        self._stream_formats = None  # set_stream_formats' names (None: input_format is bank-wide)
        self.last_blocks_per_frame, self.last_stream_blocks = 0, None
        self.m_device_rate = sample_rate << log2decim  # DeviceSource::get_sample_rate(): the sink gets it >> decim
        check(ctx.lib.sdrhip_rx_create(ctx.h, nstreams, C.byref(self.cfg), C.byref(self.h)))
        self.pipelined = bool(pipelined)
        if pipelined:
            check(ctx.lib.sdrhip_rx_set_pipelined(self.h, 1))
        self.input_format, self._in_dtype = "s16", np.int16
        if input_format != "s16":
            self.set_input_format(input_format)

    def set_input_format(self, fmt):
        """"s16" | "u8" | "s8" for every later process() / submit() (sdrhip_rx_set_input_format): 8-bit input crosses the host link
        as bytes and is widened on the GPU.  Refused (SdrHipError) while async batches are filling or in flight or pipelined frames
        wait for delivery."""
        code, dt = _iq_format(fmt, ("s16", "u8", "s8"))
        check(self.ctx.lib.sdrhip_rx_set_input_format(self.h, code))
        self.input_format, self._in_dtype = fmt, dt

    def _input(self, iq):
        """the (S, n, 2) view of a process() input; 8-bit device rows padded to a multiple of 8 samples (the library's stride rule)"""
        x, is_t, squeeze = _bank_view(iq, self.nstreams, self._in_dtype)
        if is_t and self._in_dtype != np.int16 and x.shape[0] > 1 and (x.stride(0) // 2) % 8:
            x = _padded_rows(x.shape[0], x.shape[1], 8, x.dtype, x.device, src=x)
        return x, is_t, squeeze

    def error(self):
        e, self.m_error = self.m_error, ""
        return e

    def _view(self, device):
        base, stride, cnt = C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
        check(self.ctx.lib.sdrhip_rx_frames_view(self.h, C.byref(base), C.byref(stride), C.byref(cnt)))
        fb = (NB_ORIGINAL + self.nb_fec) * UDPSIZE
        return _DeviceView(base.value or 0, (self.nstreams, cnt.value, NB_ORIGINAL + self.nb_fec, UDPSIZE), (stride.value, fb, UDPSIZE, 1), device, owner=self)

    def flush_view(self, device="cuda"):
        """pipelined mode: encode and show (zero copy) the frames the last process() call completed"""
        nf = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_rx_flush(self.h, C.c_void_p(0), 0, C.byref(nf), MEM_DEVICE))
        return self._view(torch.device(device))

    def flush(self):
        """pipelined mode: -> the frames the last process() call completed, as a host array (S, n, 128 + nb_fec, 512)"""
        out, stride_bytes = _frame_buffer(self.nstreams, max(self.max_frames(0), 1), self.nb_fec)
        nf = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_rx_flush(self.h, _ptr(out), stride_bytes, C.byref(nf), MEM_HOST))
        return out[:, :nf.value]

    def last_plan(self):
        """the decimator launch of the last process() call (sdrhip_rx_last_plan)"""
        return _plan_dict(self.ctx.lib.sdrhip_rx_last_plan, self.h)

    def reconfigure(self, **kw):
        """Live change between two process() calls (sdrhip_rx_reconfigure): any of log2decim, fcpos,
        sample_bits, nb_fec, center_frequency_khz, sample_rate."""
        cfg = RxConfig(self.cfg.log2decim, self.cfg.fcpos, self.cfg.hb_variant, self.cfg.sample_bits, self.cfg.nb_fec,
                       self.cfg.center_frequency_khz, self.cfg.sample_rate)
        for k, v in kw.items():
            if k not in ("log2decim", "fcpos", "sample_bits", "nb_fec", "center_frequency_khz", "sample_rate"):
                raise TypeError("unknown rx setting %r" % k)
            setattr(cfg, k, int(v))
        check(self.ctx.lib.sdrhip_rx_reconfigure(self.h, C.byref(cfg)))
        self.cfg, self.nb_fec = cfg, cfg.nb_fec

    def set_stream_meta(self, center_frequency_khz=None, sample_rate=None):
        """Per-stream UDPSink::setCenterFrequency / setSampleRate (sdrhip_rx_set_stream_meta): sequences of nstreams values for
        the frames that later launches open; None = that field is bank-wide again (the config's value).  Never synchronises."""
        fc, _ = self._stream_ints("center_frequency_khz", center_frequency_khz, C.c_uint32, "values of 32 bits", 0, 0xffffffff)
        sr, _ = self._stream_ints("sample_rate", sample_rate, C.c_uint32, "values of 32 bits", 0, 0xffffffff)
        check(self.ctx.lib.sdrhip_rx_set_stream_meta(self.h, fc, sr))

    def stream_meta(self, stream):
        """-> {"center_frequency_khz", "sample_rate"}: what the stream's next opened frame will carry"""
        fc, sr = C.c_uint32(0), C.c_uint32(0)
        check(self.ctx.lib.sdrhip_rx_get_stream_meta(self.h, int(stream), C.byref(fc), C.byref(sr)))
        return {"center_frequency_khz": fc.value, "sample_rate": sr.value}

    def set_stream_fec(self, nb_fec=None):
        """Per-stream UDPSink::setNbBlocksFEC (sdrhip_rx_set_stream_fec): a sequence of nstreams counts, each 0..128, for the meta
        blocks later launches open and the frames they complete; None = bank-wide again (the config's nb_fec).  While it is set
        process(), submit() and pipelined mode raise, process_ragged / process_datagrams return each stream's frames as its own
        (n, 128 + nb_fec[s], 512) array, and batches whose counts differ are delivered in departure order only (set_egress).
        Refused (SdrHipError) in pipelined mode and while batches are being filled, in flight or lent."""
        arr, v = self._stream_ints("nb_fec", nb_fec, C.c_int, "counts")  # (the range is the library's to refuse)
        check(self.ctx.lib.sdrhip_rx_set_stream_fec(self.h, arr))
        self._stream_fec = v

    def stream_fec(self, stream):
        """-> (nb_fec of the stream, slot_blocks = 128 + the largest count: the pitch of the frame area's slots)"""
        r, sb = C.c_int(0), C.c_int(0)
        check(self.ctx.lib.sdrhip_rx_get_stream_fec(self.h, int(stream), C.byref(r), C.byref(sb)))
        return r.value, sb.value

    def set_stream_bits(self, bits=None):
        """Per-stream sample size (sdrhip_rx_set_stream_bits): a sequence of nstreams sizes, each 1..16 -- what every stream's
        source says in get_sample_bits() -- for the samples later launches decimate and the meta blocks they open; None = bank-wide
        again (the config's sample_bits).  While it is set process(), submit() and pipelined mode raise.  Never synchronises;
        refused (SdrHipError) in pipelined mode."""
        arr, _ = self._stream_ints("bits", bits, C.c_uint, "sizes", 0)  # (unsigned in the ABI; 1..16 is the library's to refuse)
        check(self.ctx.lib.sdrhip_rx_set_stream_bits(self.h, arr))

    def stream_bits(self, stream):
        """-> (bits of the stream, frame_bits = the sampleBits byte of the next frame it opens)"""
        b, fb = C.c_uint(0), C.c_uint(0)
        check(self.ctx.lib.sdrhip_rx_get_stream_bits(self.h, int(stream), C.byref(b), C.byref(fb)))
        return b.value, fb.value

    def set_stream_formats(self, formats=None):
        """Per-stream input format (sdrhip_rx_set_stream_format): a sequence of nstreams names, each "s16" | "u8" | "s8" -- what
        every stream's source delivers -- for the sample-fed ragged entries; None = bank-wide again (set_input_format's value).
        While it is set process(), submit() and pipelined mode raise, and process_ragged / submit_ragged take a list of S arrays
        (n_s, 2) of each stream's own dtype (packed, or laid into rows of 4-byte units, for the caller), a packed 1-D uint8 buffer
        (submit_ragged uses one from Context.host_alloc in place) or uint8 rows (S, 4 * in_stride).  The datagram entries ignore
        it.  Never synchronises; refused (SdrHipError) in pipelined mode and while batches are being filled or in flight."""
        names = None if formats is None else list(formats)
        codes = None if names is None else [_iq_format(f, ("s16", "u8", "s8"))[0] for f in names]
        arr, _ = self._stream_ints("formats", codes, C.c_int, "formats")
        check(self.ctx.lib.sdrhip_rx_set_stream_format(self.h, arr))
        self._stream_formats = names

    def stream_format(self, stream):
        """-> "s16" | "u8" | "s8": the format the sample-fed entries read the stream's rows in"""
        f = C.c_int(0)
        check(self.ctx.lib.sdrhip_rx_get_stream_format(self.h, int(stream), C.byref(f)))
        return [k for k, v in _IQ_FORMATS.items() if v[0] == f.value][0]

    def _formatted_input(self, iq, counts, packed):
        """an input of the ragged entries while set_stream_formats' array is set -> (uint8 buffer, counts, in_stride in 4-byte
        units (0 = packed), whether it is a torch tensor).  packed: the entry takes packed rows (submit_ragged); otherwise a
        list or a packed buffer is laid into rows"""
        S, fm = self.nstreams, self._stream_formats
        bps = np.array([4 if f == "s16" else 2 for f in fm], dtype=np.int64)
        if isinstance(iq, (list, tuple)):
            if len(iq) != S:
                raise ValueError("one array per stream")
            rows = []
            for s, a in enumerate(iq):
                a = np.asarray(a)
                if a.dtype != _IQ_FORMATS[fm[s]][1] or a.ndim != 2 or a.shape[1] != 2:
                    raise TypeError("stream %d: (n, 2) of %s expected" % (s, np.dtype(_IQ_FORMATS[fm[s]][1]).name))
                rows.append(np.ascontiguousarray(a))
            cnt = np.asarray([r.shape[0] for r in rows] if counts is None else counts, dtype=np.int64).reshape(-1)
            if cnt.shape[0] != S or any(c < 0 or c > r.shape[0] for c, r in zip(cnt, rows)):
                raise ValueError("counts: one per stream, each within its array")
            parts = [rows[s][:cnt[s]].reshape(-1).view(np.uint8) for s in range(S)]
            flat = np.concatenate(parts) if S else np.zeros(0, np.uint8)
        else:
            is_t = _is_torch(iq)
            a = iq if is_t else np.asarray(iq)
            if a.dtype != (torch.uint8 if is_t else np.uint8) or a.ndim not in (1, 2):
                raise TypeError("a list of per-stream arrays, a packed 1-D uint8 buffer or uint8 rows (S, 4 * in_stride) expected")
            if a.ndim == 2:  # rows in place: row s holds counts[s] samples of its format at its start
                row_bytes = a.stride(0) if is_t else a.strides[0]
                if a.shape[0] != S or row_bytes % 4 or (a.stride(1) if is_t else a.strides[1]) != 1:
                    raise ValueError("uint8 rows: (%d, 4 * in_stride), bytes contiguous" % S)
                cnt = _counts(counts, S, a.shape[1] // 2)
                if S and int((cnt * bps).max()) > a.shape[1]:
                    raise ValueError("a row is shorter than its count takes")
                return a, cnt, max(row_bytes // 4, 1), is_t
            if is_t:
                raise TypeError("packed input is host memory")
            flat = np.ascontiguousarray(a)
            cnt = _counts(counts, S, flat.size // 2)
            if int((cnt * bps).sum()) != flat.size:
                raise ValueError("packed input holds %d bytes, the counts take %d" % (flat.size, int((cnt * bps).sum())))
        if packed:
            return flat, cnt, 0, False
        stride = max((int(cnt.max()) + 3) & ~3, 4) if S else 4
        buf, off = np.zeros((S, 4 * stride), np.uint8), 0
        for s in range(S):
            n = int(cnt[s] * bps[s])
            buf[s, :n] = flat[off:off + n]
            off += n
        return buf, cnt, stride, False

    def _stream_ints(self, name, values, ctype, what, lo=None, hi=None):
        """a per-stream setter's argument: a sequence of nstreams ints, each lo..hi where a bound is given -> (its ctypes array, the
        ints); None (bank-wide again) -> (None, None)"""
        if values is None:
            return None, None
        v = [int(x) for x in values]
        if len(v) != self.nstreams or any((lo is not None and x < lo) or (hi is not None and x > hi) for x in v):
            raise ValueError("%s: %d %s, one per stream" % (name, self.nstreams, what))
        return (ctype * self.nstreams)(*v), v

    def _slot_fec(self):
        """the count that sizes a frame slot and a delivery row: the largest of set_stream_fec's array, else nb_fec"""
        return max(self._stream_fec) if self._stream_fec else self.nb_fec

    def _stream_frames(self, out, nf):
        """set_stream_fec's delivery: row s of `out` holds stream s's nf[s] frames dense, 128 + nb_fec[s] super blocks each"""
        res = []
        for s, r in enumerate(self._stream_fec):
            n = int(nf[s]) * (NB_ORIGINAL + r) * UDPSIZE
            res.append(out[s].reshape(-1)[:n].reshape(int(nf[s]), NB_ORIGINAL + r, UDPSIZE))
        return res

    def set_follow_meta(self, on=True):
        """Outgoing meta from the incoming meta blocks (sdrhip_rx_set_follow_meta), for process_datagrams / submit_datagrams: a
        stream whose collector holds a meta block with a sample rate other than 0 announces that block's centre frequency and its
        rate >> log2decim in the frames later calls and submits open; the others keep the host's values.  A host flag: never
        synchronises, a batch in flight keeps the mode of its submit.  stream_meta() keeps reporting the host's values: the
        followed ones are in the delivered frames, and in collector_stats(s)["output_meta"]."""
        check(self.ctx.lib.sdrhip_rx_set_follow_meta(self.h, 1 if on else 0))

    def set_follow_bits(self, on=True):
        """The sample size from the incoming meta blocks (sdrhip_rx_set_follow_bits), for process_datagrams / submit_datagrams: a
        stream whose collector holds a meta block that says a sample size b of 1..16 decimates with the shift of (log2decim, b) and
        announces the decimated size in the frames later calls and submits open; the others keep the host's size (set_stream_bits,
        else sample_bits).  A host flag, independent of set_follow_meta: never synchronises, a batch in flight keeps the mode of its
        submit.  stream_bits() keeps reporting the host's values: the followed ones are in the delivered frames."""
        check(self.ctx.lib.sdrhip_rx_set_follow_bits(self.h, 1 if on else 0))

    def follow_testsource(self, ts):
        """What sdrdaemonrx's loop does with its source, per stream of a TestSource bank: setCenterFrequency(frequency / 1000)
        and setSampleRate(srate >> decim) (sdrdaemonrx.cpp:597,624,644)"""
        if ts.nstreams != self.nstreams:
            raise ValueError("the TestSource bank has %d streams, the pipe %d" % (ts.nstreams, self.nstreams))
        g = [ts.get(s) for s in range(self.nstreams)]
        self.set_stream_meta([x["frequency"] // 1000 for x in g], [x["sample_rate"] >> self.cfg.log2decim for x in g])

    def configure(self, m):
        """The control-message keys of sdrdaemonrx (parsekv pairs): decim, fcpos (Downsampler.cpp:32-67),
        fecblk (UDPSink::setNbBlocksFEC), freq in Hz (setCenterFrequency: kHz on the wire), srate
        (sample rate of the device: the sink gets srate >> decim, sdrdaemonrx.cpp:622-631).  Returns False
        on an invalid value, like Downsampler::configure; unknown keys belong to other components."""
        kw = {}
        try:
            if "decim" in m:
                kw["log2decim"] = int(m["decim"])
            if "fcpos" in m:
                kw["fcpos"] = int(m["fcpos"])
            if "fecblk" in m:
                kw["nb_fec"] = int(m["fecblk"])
            if "freq" in m:
                kw["center_frequency_khz"] = int(m["freq"]) // 1000
            if "srate" in m:
                self.m_device_rate = int(m["srate"])
            if "srate" in m or "decim" in m:
                # the reference recomputes get_sample_rate() / (1 << decim) for every block (sdrdaemonrx.cpp:640-644)
                kw["sample_rate"] = self.m_device_rate >> kw.get("log2decim", self.cfg.log2decim)
            if kw:
                self.reconfigure(**kw)
        except (ValueError, SdrHipError) as e:
            self.m_error = str(e)
            return False
        return True

    def max_frames(self, n_in):
        return self.ctx.lib.sdrhip_rx_max_frames(self.h, n_in)

    # ---- asynchronous host-pointer entry (sdrhip_rx_submit / sdrhip_rx_collect)
    def set_async(self, depth=4, blocks=1):
        """ring of `depth` batches, `blocks` submitted blocks per upload + launch + download"""
        check(self.ctx.lib.sdrhip_rx_set_async(self.h, depth, blocks))
        self._log.reset(blocks)

    def submit(self, iq, tv_sec=0, tv_usec=0):
        """one block of host samples per stream (numpy; memory from Context.host_alloc is used in place); returns at once.
        Raises SdrHipError(code SDRHIP_EBUSY = -6) when every batch of the ring is in flight."""
        if _is_torch(iq):
            raise TypeError("submit takes host memory")
        a = np.asarray(iq)
        if _rows_in_place(a, self.nstreams, self._in_dtype):
            x = a
        else:
            x, _, _ = _bank_view(iq, self.nstreams, self._in_dtype)
        check(self.ctx.lib.sdrhip_rx_submit(self.h, _ptr(x), x.shape[1], _stride_samples(x), tv_sec, tv_usec))
        if x.shape[1]:
            self._log.block("uniform", x.shape[1], self.nb_fec)

    def collect(self, wait=True, max_frames=None):
        """-> the finished frames of the oldest batch (S, n, 128 + nb_fec, 512; n may be 0), or None when no batch was collected:
        nothing submitted, or (wait = False) the oldest batch is still in flight / being filled"""
        # (the frames have the size in force when the batch was launched, whatever reconfigure() has set since; the buffer is sized
        # from the batches at hand, not from a lifetime total)
        _, nb_fec = self._log.head(self.nb_fec, "uniform" if wait else None)
        cap = max_frames if max_frames is not None else max(self._log.sample_room() // (SAMPLES_PER_FRAME << self.cfg.log2decim) + 2, 1)
        nf = C.c_size_t(0)
        for _ in range(2):  # (a batch bigger than the guess -- pipelined mode delivers the previous batch's frames -- is asked for again)
            out, stride_bytes = _frame_buffer(self.nstreams, cap, nb_fec)
            rc = self.ctx.lib.sdrhip_rx_collect(self.h, _ptr(out), stride_bytes, cap, C.byref(nf), 1 if wait else 0)
            if rc == -1 and nf.value > cap:
                cap = nf.value
                continue
            break
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        return out[:, :nf.value]

    # ---- asynchronous ragged entry (sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged)
    def submit_ragged(self, iq, counts, tv_sec=None, tv_usec=None):
        """one block per stream with its own count, returns at once.  iq: numpy rows (S, >= max(counts), 2) -- stream s takes
        counts[s] samples of row s -- or the packed samples, 1-D or (sum(counts), 2), stream after stream (memory from
        Context.host_alloc is used in place; keep it untouched until the batch is collected).  tv_sec / tv_usec: per stream or
        scalars (None = 0).  With set_stream_formats' array set iq is a list of S arrays (n_s, 2) of each stream's own dtype (packed
        for the caller; counts may be None), a packed 1-D uint8 buffer (used in place when it is Context.host_alloc memory) or uint8
        rows (S, 4 * in_stride).  Raises SdrHipError(code SDRHIP_EBUSY = -6) when every batch of the ring is in flight."""
        if _is_torch(iq):
            raise TypeError("submit_ragged takes host memory")
        S = self.nstreams
        if self._stream_formats is not None:  # (set_stream_formats: packed bytes, or uint8 rows of 4-byte units)
            a, cnt, stride, _ = self._formatted_input(iq, counts, packed=True)
            check(self.ctx.lib.sdrhip_rx_submit_ragged(self.h, _ptr(a), (C.c_size_t * S)(*cnt.tolist()), stride, _stamps(tv_sec, S),
                                                       _stamps(tv_usec, S)))
            self._log.block("ragged", cnt, self._slot_fec())
            return
        a = np.asarray(iq)
        it = np.dtype(self._in_dtype).itemsize
        if a.dtype != self._in_dtype:
            raise TypeError("numpy input must be %s" % np.dtype(self._in_dtype).name)
        if a.ndim == 3:  # rows, with their stride (rows of a bigger array are passed in place)
            if not _rows_in_place(a, S, self._in_dtype):
                a = np.ascontiguousarray(a)
                if a.shape[0] != S or a.shape[2] != 2:
                    raise ValueError("expected shape (%d, n, 2)" % S)
            cnt = _counts(counts, S, a.shape[1])
            stride = a.strides[0] // (2 * it) if a.shape[1] else 0
            if stride < (int(cnt.max()) if S else 0):
                raise ValueError("rows shorter than the largest count")
            stride = max(stride, 1)
        elif a.ndim in (1, 2):  # packed
            if a.ndim == 2 and a.shape[1] != 2:
                raise ValueError("packed input: (sum(counts), 2) or 1-D")
            a = np.ascontiguousarray(a)
            cnt = _counts(counts, S, a.size // 2)
            if int(cnt.sum()) * 2 != a.size:
                raise ValueError("packed input holds %d samples, the counts sum to %d" % (a.size // 2, int(cnt.sum())))
            stride = 0  # SDRHIP_PACKED
        else:
            raise ValueError("expected rows (%d, n, 2) or packed samples" % S)
        check(self.ctx.lib.sdrhip_rx_submit_ragged(self.h, _ptr(a), (C.c_size_t * S)(*cnt.tolist()), stride, _stamps(tv_sec, S),
                                                   _stamps(tv_usec, S)))
        self._log.block("ragged", cnt, self._slot_fec())

    def collect_ragged(self, wait=True, max_frames=None):
        """-> the frames of the oldest ragged batch: a list of S arrays (n_s, 128 + nb_fec, 512), n_s possibly 0; None when no
        batch was collected (nothing submitted, or with wait = False the oldest batch is still in flight / being filled)"""
        S = self.nstreams
        rec, nb_fec = self._log.head(self.nb_fec, "ragged" if wait else None)
        oldest = rec or self._log.filling
        cap = max_frames if max_frames is not None else (oldest.most if oldest else 0) // (SAMPLES_PER_FRAME << self.cfg.log2decim) + 2
        cap = max(cap, 1)
        nf = (C.c_size_t * S)()
        for _ in range(2):  # (a batch bigger than the guess is asked for again with room for its largest stream)
            out, stride_bytes = _frame_buffer(S, cap, nb_fec)
            rc = self.ctx.lib.sdrhip_rx_collect_ragged(self.h, _ptr(out), stride_bytes, cap, nf, 1 if wait else 0)
            if rc == -1 and max_frames is None and S and max(nf[:]) > cap:
                cap = max(nf[:])
                continue
            break
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        return [out[s, :nf[s]] for s in range(S)]

    def process(self, iq, tv_sec=0, tv_usec=0, out=None):
        """-> frames (S, n_frames, 128 + nb_fec, 512) uint8 (squeezed for one stream)"""
        x, is_t, squeeze = self._input(iq)
        S, n = x.shape[0], x.shape[1]
        out, stride_bytes = _frame_buffer(S, max(self.max_frames(n), 1), self.nb_fec, x.device if is_t else None, out)
        nf = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_rx_process(self.h, _ptr(x), n, _stride_samples(x), tv_sec, tv_usec, _ptr(out), stride_bytes,
                                             C.byref(nf), MEM_DEVICE if is_t else MEM_HOST))
        out = out[:, :nf.value]
        return out[0] if squeeze else out

    def process_view(self, iq, tv_sec=0, tv_usec=0):
        """Zero-copy variant for CUDA tensors: the finished frames stay in the library's frame area.
        -> uint8 CUDA tensor view (S, n_frames, 128 + nb_fec, 512), valid until the next process call."""
        x, is_t, squeeze = self._input(iq)
        if not is_t:
            raise TypeError("process_view needs a CUDA tensor")
        S, n = x.shape[0], x.shape[1]
        nf = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_rx_process(self.h, _ptr(x), n, _stride_samples(x), tv_sec, tv_usec, C.c_void_p(0), 0,
                                             C.byref(nf), MEM_DEVICE))
        return self._view(x.device)

    def _ragged_input(self, iq):
        """_input, with int16 device rows padded to a multiple of 4 samples as well (the library's stride rule).  NOTE: a CUDA
        tensor whose row stride is not a multiple of 4 samples is COPIED whole into a padded buffer on every call; pass rows
        allocated with such a stride to avoid the copy."""
        x, is_t, squeeze = self._input(iq)
        if is_t and x.shape[0] > 1 and (x.stride(0) // 2) % 4:
            x = _padded_rows(x.shape[0], x.shape[1], 4, x.dtype, x.device, src=x)
        return x, is_t, squeeze

    def _ragged_args(self, x, counts, tv_sec, tv_usec):
        S = x.shape[0]
        cnt = _counts(counts, S, x.shape[1])
        return cnt, (C.c_size_t * S)(*cnt.tolist()), _stamps(tv_sec, S), _stamps(tv_usec, S)

    def process_ragged(self, iq, counts, tv_sec=0, tv_usec=0, out=None):
        """sdrhip_rx_process_ragged: stream s takes counts[s] samples of row s of iq (S, >= max(counts), 2), stamped tv_sec[s] /
        tv_usec[s] (scalars apply to every stream).  -> (frames (S, max_frames, 128 + nb_fec, 512) uint8, n_frames numpy (S,)):
        stream s's frames are frames[s, :n_frames[s]].  With set_stream_fec's array set: (a list of S arrays (n_frames[s],
        128 + nb_fec[s], 512), n_frames).  With set_stream_formats' array set iq is a list of S arrays (n_s, 2) of each stream's own
        dtype (counts may be None: every array whole), a packed 1-D uint8 buffer, or uint8 rows (S, 4 * in_stride), numpy or CUDA."""
        if self._stream_formats is not None:  # (set_stream_formats: uint8 rows of 4-byte units, each stream in its own format)
            x, cnt, in_stride, is_t = self._formatted_input(iq, counts, packed=False)
            S = self.nstreams
            c_cnt, c_sec, c_usec = (C.c_size_t * S)(*cnt.tolist()), _stamps(tv_sec, S), _stamps(tv_usec, S)
        else:
            x, is_t, _ = self._ragged_input(iq)
            S, in_stride = x.shape[0], _stride_samples(x)
            cnt, c_cnt, c_sec, c_usec = self._ragged_args(x, counts, tv_sec, tv_usec)
        cap = max(self.max_frames(int(cnt.max()) if S else 0), 1)
        out, stride_bytes = _frame_buffer(S, cap, self._slot_fec(), x.device if is_t else None, out)
        nf = (C.c_size_t * S)()
        check(self.ctx.lib.sdrhip_rx_process_ragged(self.h, _ptr(x), c_cnt, in_stride, c_sec, c_usec, _ptr(out),
                                                    stride_bytes, nf, MEM_DEVICE if is_t else MEM_HOST))
        n_frames = np.array(nf[:], dtype=np.int64)
        if self._stream_fec is not None:
            return self._stream_frames(out, nf), n_frames
        return out[:, :int(n_frames.max()) if S else 0], n_frames

    def frames_view_ragged(self, device="cuda"):
        """the frames the last call delivered (sdrhip_rx_frames_view_ragged): a list of S uint8 CUDA tensors (n_frames[s], 128 + nb_fec,
        512) sharing the library's frame area, valid until the next call on this pipe"""
        S = self.nstreams
        base, stride = C.c_void_p(0), C.c_size_t(0)
        first, cnt = (C.c_size_t * S)(), (C.c_size_t * S)()
        check(self.ctx.lib.sdrhip_rx_frames_view_ragged(self.h, C.byref(base), C.byref(stride), first, cnt))
        fb = (NB_ORIGINAL + self._slot_fec()) * UDPSIZE  # (the slot pitch; with set_stream_fec a frame shows its own 128 + nb_fec[s] blocks)
        rows = [NB_ORIGINAL + (self._stream_fec[s] if self._stream_fec else self.nb_fec) for s in range(S)]
        dev = torch.device(device)
        return [_DeviceView((base.value or 0) + s * stride.value + first[s] * fb, (cnt[s], rows[s], UDPSIZE),
                            (fb, UDPSIZE, 1), dev, owner=self).torch() if cnt[s] else
                torch.empty((0, rows[s], UDPSIZE), dtype=torch.uint8, device=dev) for s in range(S)]

    def process_view_ragged(self, iq, counts, tv_sec=0, tv_usec=0):
        """Zero-copy ragged call for CUDA tensors: -> (list of S frame tensors as frames_view_ragged, n_frames numpy (S,))"""
        if self._stream_formats is not None:  # (set_stream_formats: uint8 device rows (S, 4 * in_stride))
            x, cnt, in_stride, is_t = self._formatted_input(iq, counts, packed=False)
            S = self.nstreams
            c_cnt, c_sec, c_usec = (C.c_size_t * S)(*cnt.tolist()), _stamps(tv_sec, S), _stamps(tv_usec, S)
        else:
            x, is_t, _ = self._ragged_input(iq)
            S, in_stride = x.shape[0], _stride_samples(x)
            _, c_cnt, c_sec, c_usec = self._ragged_args(x, counts, tv_sec, tv_usec)
        if not is_t:
            raise TypeError("process_view_ragged needs a CUDA tensor")
        nf = (C.c_size_t * S)()
        check(self.ctx.lib.sdrhip_rx_process_ragged(self.h, _ptr(x), c_cnt, in_stride, c_sec, c_usec, C.c_void_p(0), 0, nf,
                                                    MEM_DEVICE))
        return self.frames_view_ragged(x.device), np.array(nf[:], dtype=np.int64)

    # ---- datagram entry (sdrhip_rx_process_datagrams)
    def process_datagrams(self, dgrams_per_stream, tv_sec=0, tv_usec=0, max_released=None):
        """one (n_s, 512) uint8 array of raw FEC datagrams per stream -- numpy (host memory) or torch device tensors, as
        TxPipe.process_datagrams -- through the handle's collector, the remainder rows, the decimators, the framer and the
        encoder; tv_sec / tv_usec (scalars or one per stream) stamp the first sample each stream feeds its decimator.  -> per
        stream (frames (n, 128 + nb_fec, 512) uint8, records of the frames the collector released).  A stream that would release
        more than max_released (default: room for anything the datagrams can release) raises SdrHipError, nothing consumed;
        last_n_released has the counts."""
        S = self.nstreams
        if len(dgrams_per_stream) != S:
            raise ValueError("one datagram array per stream")
        buf, counts, is_t = _datagram_batch(dgrams_per_stream)
        if max_released is None:
            max_released = max(counts + [0])  # (a call releases at most one frame per datagram)
        F = max(max_released, 1)
        cap = max(self.max_frames(SAMPLES_PER_FRAME * max_released + 63), 1)
        out, stride_bytes = _frame_buffer(S, cap, self._slot_fec(), buf.device if is_t else None)
        info = (FECBufferFrame * (S * F))()
        nd = (C.c_size_t * S)(*counts)
        nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
        rc = self.ctx.lib.sdrhip_rx_process_datagrams(self.h, _ptr(buf), nd, buf.shape[1] * UDPSIZE, _stamps(tv_sec, S), _stamps(tv_usec, S),
                                                      max_released, _ptr(out), stride_bytes, info, nr, nf, MEM_DEVICE if is_t else MEM_HOST)
        self.last_n_released = [int(x) for x in nr]
        check(rc)
        if self._stream_fec is not None:  # (each stream's frames in its own shape, (n, 128 + nb_fec[s], 512))
            return list(zip(self._stream_frames(out, nf), _records(info, F, nr)))
        return [(out[s, :int(nf[s])], recs) for s, recs in enumerate(_records(info, F, nr))]

    # ---- asynchronous datagram batches (sdrhip_rx_submit_datagrams / sdrhip_rx_collect_datagrams)
    def submit_datagrams(self, dgrams_per_stream, tv_sec=0, tv_usec=0):
        """one batch of raw datagrams from host memory, as TxPipe.submit_datagrams takes them: one (n_s, 512) uint8 numpy array per
        stream (counts may differ, may be 0), or ONE (sum n_s, 512) array of them back to back with a list of counts as (array,
        counts) -- such an array in sdrhip_host_alloc memory goes up in place and must stay untouched until the batch is collected.
        tv_sec / tv_usec (scalars or one per stream) stamp the first sample each stream feeds its decimator in this batch.  Returns
        at once; raises SdrHipError(code SDRHIP_EBUSY = -6) when every batch of the ring is in flight."""
        S = self.nstreams
        buf, counts = _packed_datagrams(dgrams_per_stream, S)
        nd = (C.c_size_t * S)(*counts)
        check(self.ctx.lib.sdrhip_rx_submit_datagrams(self.h, _ptr(buf), nd, 0, _stamps(tv_sec, S), _stamps(tv_usec, S)))  # (0 = SDRHIP_PACKED)
        self._dg_submitted()

    def submit_datagrams_tagged(self, dgrams, stream_of, tv_sec=0, tv_usec=0):
        """one batch as a hub's socket delivers it (sdrhip_rx_submit_datagrams_tagged): dgrams (n, 512) uint8 in arrival order,
        stream_of (n,) uint16 = the stream of every datagram or DGRAM_SKIP.  It means submit_datagrams of the per-stream
        subsequences; the array goes up unsorted (from Context.host_alloc memory in place: keep it untouched until the batch is
        collected) and is demultiplexed on the device.  Collected with collect_datagrams."""
        S = self.nstreams
        buf, tags, tp = _tagged_batch(dgrams, stream_of)
        check(self.ctx.lib.sdrhip_rx_submit_datagrams_tagged(self.h, _ptr(buf), tp, buf.shape[0], _stamps(tv_sec, S), _stamps(tv_usec, S)))
        self._dg_submitted()

    def _dg_submitted(self):
        """a datagram batch was submitted (also for callers of the C entry itself): the log's record of it, with the nb_fec it keeps"""
        self._log.batch("datagram", None, self._slot_fec())

    def collect_datagrams(self, wait=True, max_frames=None, max_released=None):
        """the oldest datagram batch: per stream (frames (n, 128 + nb_fec, 512) uint8, records) as process_datagrams returns them, or
        None when no batch was collected (nothing submitted, or wait=False and the oldest one is in flight).  max_frames /
        max_released = None: room for exactly what the batch holds (one call that learns the counts, one that collects); a batch
        that holds more than a given bound raises SdrHipError and stays (last_n_frames / last_n_released have the counts)."""
        S = self.nstreams
        nr, nf = (C.c_size_t * S)(), (C.c_size_t * S)()
        w = 1 if wait else 0
        _, nb_fec = self._log.head(self.nb_fec)
        if max_frames is None or max_released is None:
            rc = self.ctx.lib.sdrhip_rx_collect_datagrams(self.h, None, 0, 0, 0, None, nr, nf, w)
            if rc == -6:
                return None
            if rc == 0:  # (a batch that released and completed nothing: collected)
                self._log.pop()
                self.last_n_released, self.last_n_frames = [0] * S, [0] * S
                return [(np.zeros((0, NB_ORIGINAL + nb_fec, UDPSIZE), np.uint8), []) for _ in range(S)]
            if rc != -1:
                check(rc)
            if max_frames is None:
                max_frames = max(int(x) for x in nf)
            if max_released is None:
                max_released = max(int(x) for x in nr)
        F = max(max_released, 1)
        out, stride_bytes = _frame_buffer(S, max(max_frames, 1), nb_fec)
        info = (FECBufferFrame * (S * F))()
        rc = self.ctx.lib.sdrhip_rx_collect_datagrams(self.h, _ptr(out), stride_bytes, max_frames, max_released, info, nr, nf, w)
        self.last_n_released, self.last_n_frames = [int(x) for x in nr], [int(x) for x in nf]
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        return [(out[s, :int(nf[s])], recs) for s, recs in enumerate(_records(info, F, nr))]

    # ---- departure-order egress (sdrhip_rx_set_egress / sdrhip_rx_collect_egress / sdrhip_rx_release_egress)
    def set_egress(self, order="round_robin"):
        """the order later ragged and datagram batches are delivered in: "round_robin" = one array per batch, datagram j of every
        stream before datagram j + 1 of any (collect_egress); "paced" = one array in ascending departure key (2j + 1) / (2 D_s),
        ties by stream -- what senders that each space their own datagrams evenly put on the wire together, so streams with
        unequal counts never burst (equal counts: the round-robin array); None or "off" = frames per stream (collect_ragged /
        collect_datagrams), the default.  A batch keeps the order it was launched with."""
        orders = {None: _lib.EGRESS_OFF, "off": _lib.EGRESS_OFF, "round_robin": _lib.EGRESS_ROUND_ROBIN, "paced": _lib.EGRESS_PACED}
        check(self.ctx.lib.sdrhip_rx_set_egress(self.h, orders[order] if order in orders else int(order)))

    def collect_egress(self, wait=True, max_released=None, copy=True):
        """the oldest batch launched with an egress order -> (dgrams (n, 512) uint8 in departure order, stream_of (n,) uint16,
        n_frames numpy (S,), records), or None when no batch was collected (nothing submitted, or wait=False and the oldest one is
        in flight).  records: per stream the records of the frames its collector released, as collect_datagrams returns them;
        None for a ragged batch.  blocks per frame of the batch: last_blocks_per_frame -- 0 for a batch whose streams' counts
        differ (set_stream_fec), last_stream_blocks then lists every stream's (else it is None).  copy=False returns views of the memory
        the library lends -- the batch's pinned download buffer and its tags -- valid until release_egress, the next
        collect_egress or the pipe's destruction; the batch keeps its ring slot meanwhile.  copy=True copies and releases."""
        S = self.nstreams
        rec, _ = self._log.head(self.nb_fec, "ragged" if wait else None)
        is_dg = rec is not None and rec.kind == "datagram"
        eg = _lib.RxEgress()
        nf, nr = (C.c_size_t * S)(), (C.c_size_t * S)()
        F, info = (max_released or 0), None
        for _ in range(2):  # (max_released=None: one call that learns the counts, one that collects)
            info = (FECBufferFrame * (S * F))() if F else None
            rc = self.ctx.lib.sdrhip_rx_collect_egress(self.h, C.byref(eg), nf, F, info, nr, 1 if wait else 0)
            if rc == -1 and max_released is None and S and max(nr[:]) > F:
                F = max(nr[:])
                continue
            break
        self.last_n_released, self.last_n_frames = [int(x) for x in nr], [int(x) for x in nf]
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        n = int(eg.n_dgrams)
        self.last_blocks_per_frame = int(eg.blocks_per_frame)
        self.last_stream_blocks = None
        if n and not self.last_blocks_per_frame:
            sb = (C.c_size_t * S)()
            check(self.ctx.lib.sdrhip_rx_egress_stream_blocks(self.h, sb))
            self.last_stream_blocks = [int(x) for x in sb]
        if n:
            dg = np.ctypeslib.as_array((C.c_uint8 * (n * UDPSIZE)).from_address(eg.dgrams)).reshape(n, UDPSIZE)
            tags = np.ctypeslib.as_array((C.c_uint16 * n).from_address(eg.stream_of))
        else:
            dg, tags = np.zeros((0, UDPSIZE), np.uint8), np.zeros(0, np.uint16)
        if copy:
            dg, tags = dg.copy(), tags.copy()
            self.release_egress()
        return dg, tags, np.array(nf[:], dtype=np.int64), _records(info, F, nr) if is_dg else None

    def release_egress(self):
        """sdrhip_rx_release_egress: the batch collect_egress(copy=False) lent is free again (its views are dead)"""
        check(self.ctx.lib.sdrhip_rx_release_egress(self.h))

    def collector_stats(self, stream):
        """the statistics of one stream's collector (sdrhip_rx_collector + sdrhip_fecbuf_stats): the dict of FECBufferBank.stats"""
        return _fecbuf_stats(self.ctx, self._collector(), stream)

    def reset_streams(self, streams=None):
        """sdrhip_rx_reset_streams: the streams listed (None: every stream, the whole-pipe reset) begin again as a restarted
        sdrdaemonrx does -- zero decimator histories, the open frame dropped, m_frameCount 0, a fresh collector and no carry --
        while the others run on.  One small launch, no synchronisation."""
        check(self.ctx.lib.sdrhip_rx_reset_streams(self.h, _stream_mask(streams, self.nstreams)))

    def export_stream(self, stream):
        """sdrhip_rx_export_stream: the state of one stream as opaque bytes (histories, open frame, collector, held-back samples);
        the source is left untouched.  Synchronises once."""
        return _export_stream(self.ctx, "rx", self.h, stream)

    def import_stream(self, stream, blob):
        """sdrhip_rx_import_stream: stream `stream` of this bank continues where the exported stream stood, under this bank's
        own configuration; the bank's other streams run on.  One upload, one launch, no synchronisation."""
        _import_stream(self.ctx, "rx", self.h, stream, blob)

    def reset_collector(self):
        """sdrhip_fecbuf_reset on the handle's collector: the constructor's state, and every stream's carry cleared"""
        check(self.ctx.lib.sdrhip_fecbuf_reset(self._collector()))

    def _collector(self):
        h = C.c_void_p()
        check(self.ctx.lib.sdrhip_rx_collector(self.h, C.byref(h)))
        return h

    def carry(self):
        """samples each stream holds back between process_datagrams calls (sdrhip_rx_carry): numpy (S,)"""
        c = (C.c_size_t * self.nstreams)()
        check(self.ctx.lib.sdrhip_rx_carry(self.h, c))
        return np.array(c[:], dtype=np.int64)


class TxPipe(_Handle):
    """SDRdaemonFECBuffer decode -> Upsampler for a bank of streams (sdrhip_tx).  pipelined=True: process() decodes its batch
    on the context's second stream while the previous batch is interpolated, and returns the PREVIOUS batch's samples
    (sdrhip_tx_set_pipelined); flush() returns the last batch's at the end.  A device-memory rx batch must stay untouched until
    the next process() / flush() has returned."""

    _destroy = "sdrhip_tx_destroy"

    def __init__(self, ctx, nstreams=1, log2interp=4, pipelined=False, output_format="s16"):
        """output_format: "s16" (int16 IQ) or "s8" (HackRF int8), see set_output_format"""
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams, self.log2interp = ctx, nstreams, log2interp
        self._log = _BatchLog()  # the asynchronous batches in flight, each with the log2interp it keeps (the collects size with it)
        self.m_error = ""
        self.pipelined = bool(pipelined)
        check(ctx.lib.sdrhip_tx_create(ctx.h, nstreams, log2interp, C.byref(self.h)))
        if pipelined:
            check(ctx.lib.sdrhip_tx_set_pipelined(self.h, 1))
        self.output_format, self._out_dtype = "s16", np.int16
        self._stream_formats = None
        if output_format != "s16":
            self.set_output_format(output_format)

    def set_output_format(self, fmt):
        """"s16" | "s8" for every later process() / flush() / collect() / process_datagrams() (sdrhip_tx_set_output_format): with
        "s8" the samples come back as int8 (v >> 8 of each component, narrowed on the GPU).  Refused (SdrHipError) while async
        batches are in flight or a pipelined batch waits."""
        code, dt = _iq_format(fmt, ("s16", "s8"))
        check(self.ctx.lib.sdrhip_tx_set_output_format(self.h, code))
        self.output_format, self._out_dtype = fmt, dt

    def set_stream_formats(self, formats=None):
        """Per-stream output format (sdrhip_tx_set_stream_format): a sequence of nstreams names, each "s16" | "s8" -- what every
        stream's sink takes (int16 file / HackRF bytes) -- for every later entry; None = bank-wide again (set_output_format's
        value).  While it is set every entry returns a LIST with one array per stream, (n, 2) int8 or int16, where the bank-wide
        handle returns one (S, n, 2) array.  Never synchronises; refused (SdrHipError) while async batches are in flight or a
        pipelined batch waits."""
        names = None if formats is None else list(formats)
        arr = None
        if names is not None:
            if len(names) != self.nstreams:
                raise ValueError("formats: %d names, one per stream" % self.nstreams)
            arr = (C.c_int * self.nstreams)(*[_iq_format(f, ("s16", "s8"))[0] for f in names])
        check(self.ctx.lib.sdrhip_tx_set_stream_format(self.h, arr))
        self._stream_formats = names

    def stream_format(self, stream):
        """-> "s16" | "s8": the format the stream's samples are delivered in"""
        f = C.c_int(0)
        check(self.ctx.lib.sdrhip_tx_get_stream_format(self.h, int(stream), C.byref(f)))
        return [k for k, v in _IQ_FORMATS.items() if v[0] == f.value][0]

    def _rows(self, out, counts):
        """what an entry returns for the buffer of _out: bank-wide, out[:, :counts] (counts an int) -- or, with set_stream_formats'
        array set, the list of every stream's own (counts[s], 2) array of its dtype (counts an int or one per stream)"""
        fm = self._stream_formats
        if fm is None:
            return out[:, :counts]
        n = [counts] * self.nstreams if isinstance(counts, int) else list(counts)
        res = []
        for s, f in enumerate(fm):
            b = out[s, :n[s] * (4 if f == "s16" else 2)]
            if _is_torch(out):
                res.append(b.view(torch.int16 if f == "s16" else torch.int8).reshape(n[s], 2))
            else:
                res.append(b.view(_IQ_FORMATS[f][1]).reshape(n[s], 2))
        return res

    def _out(self, S, n_res, device=None):
        """output buffer of (S, pitch, 2) samples: rows of a multiple of 4 (int16) / 8 (int8) samples, the library's stride rule.
        (set_stream_formats' array set: (S, 4 * pitch) bytes, the pitch a multiple of 4 of its 4-byte units; _rows reads it)"""
        if self._stream_formats is not None:
            pad = max((n_res + 3) & ~3, 4)
            return (torch.empty((S, 4 * pad), dtype=torch.uint8, device=device) if device is not None else np.empty((S, 4 * pad), np.uint8)), pad
        if self._out_dtype == np.int16:
            pad = max((n_res + 3) & ~3, 4)
            return (torch.empty((S, pad, 2), dtype=torch.int16, device=device) if device is not None else np.empty((S, pad, 2), np.int16)), pad
        pad = max((n_res + 7) & ~7, 8)
        return (torch.empty((S, pad, 2), dtype=torch.int8, device=device) if device is not None else np.empty((S, pad, 2), np.int8)), pad

    def configure(self, m):
        """The `interp` key of a control message (Upsampler::configure, Upsampler.cpp:31-50) between two batches;
        -> bool, the message is kept for error()."""
        if "interp" in m:
            try:
                check(self.ctx.lib.sdrhip_tx_reconfigure(self.h, int(m["interp"])))
                self.log2interp = int(m["interp"])
            except (ValueError, SdrHipError) as e:
                self.m_error = str(e)
                return False
        return True

    def error(self):
        e, self.m_error = self.m_error, ""
        return e

    def process(self, rx, indices=None):
        """rx (S, F, 128, 512) uint8 (or (F, 128, 512)) -> iq (S, F*16129 << log2interp, 2) int16"""
        is_t = _is_torch(rx)
        squeeze = rx.ndim == 3
        if squeeze:
            rx = rx[None]
        S, F = rx.shape[0], rx.shape[1]
        if not is_t:
            rx = np.ascontiguousarray(rx, dtype=np.uint8)
        else:
            rx = rx.contiguous()
        if indices is not None:  # optional (see fec_decode_frames)
            indices = np.ascontiguousarray(indices, dtype=np.uint8)
        n_res = (F * SAMPLES_PER_FRAME) << self.log2interp
        if self.pipelined:  # (the call delivers the batch the PREVIOUS call decoded)
            n_res = self.ctx.lib.sdrhip_tx_pending_samples(self.h)
        out, pad = self._out(S, n_res, rx.device if is_t else None)
        n_out = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_tx_process(self.h, _ptr(rx), C.c_void_p(indices.ctypes.data if indices is not None else 0), F, F * NB_ORIGINAL * UDPSIZE,
                                             _ptr(out), pad, C.byref(n_out), MEM_DEVICE if is_t else MEM_HOST))
        out = self._rows(out, n_out.value if self.pipelined else n_res)
        return out[0] if squeeze else out

    # ---- asynchronous host-pointer entry (sdrhip_tx_submit / sdrhip_tx_collect)
    def set_async(self, depth=4):
        """ring of `depth` batches in flight"""
        check(self.ctx.lib.sdrhip_tx_set_async(self.h, depth))
        self._log.reset()

    def submit(self, rx, indices=None):
        """one batch of received frames from host memory, (S, F, 128, 512) uint8 (or (F, 128, 512)); returns at once.  Raises
        SdrHipError(code SDRHIP_EBUSY = -6) when every batch of the ring is in flight."""
        if _is_torch(rx):
            raise TypeError("submit takes host memory")
        a = np.asarray(rx)
        if a.ndim == 3:
            a = a[None]
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[0] != self.nstreams or a.shape[2:] != (NB_ORIGINAL, UDPSIZE):
            raise ValueError("expected (%d, F, 128, 512) uint8" % self.nstreams)
        if not (a.strides[3] == 1 and a.strides[2] == UDPSIZE and a.strides[1] == NB_ORIGINAL * UDPSIZE):
            a = np.ascontiguousarray(a)
        if indices is not None:
            indices = np.ascontiguousarray(indices, dtype=np.uint8)
        check(self.ctx.lib.sdrhip_tx_submit(self.h, _ptr(a), C.c_void_p(indices.ctypes.data if indices is not None else 0), a.shape[1], a.strides[0]))
        if a.shape[1]:
            self._log.batch("frames", a.shape[1], self.log2interp)

    def collect(self, wait=True, block0=False):
        """-> the samples of the oldest batch (S, F * 16129 << log2interp, 2) int16 -- with block0=True a pair (samples, meta blocks
        (S, F, 508) uint8) -- or None when no batch was collected (nothing submitted, or wait=False and the oldest one is in flight)"""
        rec, L = self._log.head(self.log2interp)
        F = rec.most if rec is not None else 0
        cap = max((F * SAMPLES_PER_FRAME) << L, 4)
        if self._stream_formats is not None:
            out, cap = self._out(self.nstreams, cap)
        else:
            out = np.empty((self.nstreams, cap, 2), self._out_dtype)
        b0 = np.empty((self.nstreams, max(F, 1), BLOCK_BYTES), np.uint8)
        n_out, nf = C.c_size_t(0), C.c_size_t(0)
        rc = self.ctx.lib.sdrhip_tx_collect(self.h, _ptr(out), cap, cap, _ptr(b0) if block0 else C.c_void_p(0), C.byref(n_out), C.byref(nf), 1 if wait else 0)
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        return (self._rows(out, n_out.value), b0[:, :nf.value]) if block0 else self._rows(out, n_out.value)

    def flush(self, device=None):
        """pipelined mode: the samples of the batch the last process() call decoded (sdrhip_tx_flush); (S, 0, 2) when nothing
        waits.  device: a torch device for a device-memory result, None for numpy"""
        S = self.nstreams
        n_res = self.ctx.lib.sdrhip_tx_pending_samples(self.h)
        out, pad = self._out(S, n_res, device)
        n_out = C.c_size_t(0)
        check(self.ctx.lib.sdrhip_tx_flush(self.h, _ptr(out), pad, C.byref(n_out), MEM_DEVICE if device is not None else MEM_HOST))
        return self._rows(out, n_out.value)

    # ---- datagram entry (sdrhip_tx_process_datagrams)
    def process_datagrams(self, dgrams_per_stream, max_frames=None):
        """one (n_s, 512) uint8 array of raw datagrams per stream -- numpy (host memory) or torch device tensors, as
        FECBufferBank.write_and_read -- through the handle's collector and interpolators; -> per stream (iq (n, 2) int16 with
        n = frames * 16129 << log2interp, block0 (frames, 508) uint8, records)"""
        S = self.nstreams
        if len(dgrams_per_stream) != S:
            raise ValueError("one datagram array per stream")
        buf, counts, is_t = _datagram_batch(dgrams_per_stream)
        if max_frames is None:
            max_frames = max(counts + [0])  # (a call releases at most one frame per datagram)
        F = max(max_frames, 1)
        n_cap = (F * SAMPLES_PER_FRAME) << self.log2interp
        out, pad = self._out(S, n_cap, buf.device if is_t else None)
        if is_t:
            b0 = torch.empty((S, F, BLOCK_BYTES), dtype=torch.uint8, device=buf.device)
        else:
            b0 = np.empty((S, F, BLOCK_BYTES), np.uint8)
        info = (FECBufferFrame * (S * F))()
        nd = (C.c_size_t * S)(*counts)
        nf = (C.c_size_t * S)()
        rc = self.ctx.lib.sdrhip_tx_process_datagrams(self.h, _ptr(buf), nd, buf.shape[1] * UDPSIZE, _ptr(out), pad, max_frames, _ptr(b0),
                                                      info, nf, MEM_DEVICE if is_t else MEM_HOST)
        self.last_n_frames = [int(x) for x in nf]
        check(rc)
        return self._dg_result(out, b0, _records(info, F, nf), self.log2interp)

    def _dg_result(self, out, b0, records, L):
        """per stream (iq, block0, records) of a datagram entry: each stream's own samples, in its own dtype while formats are set"""
        n = [(len(recs) * SAMPLES_PER_FRAME) << L for recs in records]
        iq = self._rows(out, n) if self._stream_formats is not None else [out[s, :n[s]] for s in range(len(n))]
        return [(iq[s], b0[s, :len(recs)], recs) for s, recs in enumerate(records)]

    # ---- asynchronous datagram batches (sdrhip_tx_submit_datagrams / sdrhip_tx_collect_datagrams)
    def submit_datagrams(self, dgrams_per_stream):
        """one batch of raw datagrams from host memory: one (n_s, 512) uint8 numpy array per stream (counts may differ, may be 0),
        or ONE (sum n_s, 512) array of them back to back with a list of counts as (array, counts) -- such an array in
        sdrhip_host_alloc memory goes up in place and must stay untouched until the batch is collected.  Returns at once; raises
        SdrHipError(code SDRHIP_EBUSY = -6) when every batch of the ring is in flight."""
        S = self.nstreams
        buf, counts = _packed_datagrams(dgrams_per_stream, S)
        nd = (C.c_size_t * S)(*counts)
        check(self.ctx.lib.sdrhip_tx_submit_datagrams(self.h, _ptr(buf), nd, 0))  # (0 = SDRHIP_PACKED)
        self._log.batch("datagram", None, self.log2interp)

    def submit_datagrams_tagged(self, dgrams, stream_of):
        """one batch as a hub's socket delivers it (sdrhip_tx_submit_datagrams_tagged): dgrams (n, 512) uint8 in arrival order,
        stream_of (n,) uint16 = the stream of every datagram or DGRAM_SKIP.  It means submit_datagrams of the per-stream
        subsequences; the array goes up unsorted (from Context.host_alloc memory in place) and is demultiplexed on the device.
        Collected with collect_datagrams."""
        buf, tags, tp = _tagged_batch(dgrams, stream_of)
        check(self.ctx.lib.sdrhip_tx_submit_datagrams_tagged(self.h, _ptr(buf), tp, buf.shape[0]))
        self._log.batch("datagram", None, self.log2interp)

    def collect_datagrams(self, wait=True, max_frames=None):
        """the oldest datagram batch: per stream (iq (n, 2) with n = frames * 16129 << the batch's log2interp, block0 (frames, 508)
        uint8, records) as process_datagrams returns them, or None when no batch was collected (nothing submitted, or wait=False
        and the oldest one is in flight).  max_frames=None: room for exactly what the batch released (one call that learns the
        counts, one that collects)."""
        S = self.nstreams
        nf = (C.c_size_t * S)()
        if max_frames is None:
            rc = self.ctx.lib.sdrhip_tx_collect_datagrams(self.h, None, 0, 0, None, None, nf, 1 if wait else 0)
            if rc == -6:
                return None
            if rc == 0:  # (a batch that released nothing: collected)
                self._log.pop()
                dts = [self._out_dtype] * S if self._stream_formats is None else [_IQ_FORMATS[f][1] for f in self._stream_formats]
                return [(np.zeros((0, 2), dt), np.zeros((0, BLOCK_BYTES), np.uint8), []) for dt in dts]
            if rc != -1:
                check(rc)
            max_frames = max(int(x) for x in nf)
        _, L = self._log.head(self.log2interp)
        F = max(max_frames, 1)
        out, pad = self._out(S, (F * SAMPLES_PER_FRAME) << L)
        b0 = np.empty((S, F, BLOCK_BYTES), np.uint8)
        info = (FECBufferFrame * (S * F))()
        rc = self.ctx.lib.sdrhip_tx_collect_datagrams(self.h, _ptr(out), pad, max_frames, _ptr(b0), info, nf, 1 if wait else 0)
        self.last_n_frames = [int(x) for x in nf]
        if rc == -6:
            return None
        check(rc)
        self._log.pop()
        return self._dg_result(out, b0, _records(info, F, nf), L)

    def reset_streams(self, streams=None):
        """sdrhip_tx_reset_streams: the streams listed (None: every stream) begin again as a restarted sdrdaemontx does -- zero
        interpolator histories and a fresh collector -- while the others run on.  One small launch, no synchronisation."""
        check(self.ctx.lib.sdrhip_tx_reset_streams(self.h, _stream_mask(streams, self.nstreams)))

    def export_stream(self, stream):
        """sdrhip_tx_export_stream: the state of one stream as opaque bytes (interpolator histories, collector); the source is
        left untouched.  Synchronises once."""
        return _export_stream(self.ctx, "tx", self.h, stream)

    def import_stream(self, stream, blob):
        """sdrhip_tx_import_stream: stream `stream` of this bank continues where the exported stream stood; the bank's other
        streams run on.  One upload, one launch, no synchronisation."""
        _import_stream(self.ctx, "tx", self.h, stream, blob)

    def collector_stats(self, stream):
        """the statistics of one stream's collector (sdrhip_tx_collector + sdrhip_fecbuf_stats): the dict of FECBufferBank.stats"""
        h = C.c_void_p()
        check(self.ctx.lib.sdrhip_tx_collector(self.h, C.byref(h)))
        return _fecbuf_stats(self.ctx, h, stream)


class FECBufferFrame(C.Structure):
    """sdrhip_fecbuf_frame"""
    _fields_ = [("frame_index", C.c_int32), ("block_count", C.c_int32), ("recovery_count", C.c_int32), ("flags", C.c_uint32)]


FECBUF_DECODED, FECBUF_META, FECBUF_REPAIRED, FECBUF_DECODE_ERROR = 1, 2, 4, 8


class FECBufferBank(_Handle):
    """nstreams independent SDRdaemonFECBuffer collectors fed raw 512-byte datagrams (sdrhip_fecbuf).  write_and_read() takes one
    (n_s, 512) uint8 array per stream -- numpy (host memory) or torch device tensors -- and returns per stream the frames the
    datagrams released: (data (F, 127 * 508) uint8 = getSlotData, block0 (F, 508) uint8 = the meta block, records: a list of
    dicts frame_index / block_count / recovery_count / flags)."""

    _destroy = "sdrhip_fecbuf_destroy"

    def __init__(self, ctx, nstreams=1):
        _Handle.__init__(self, ctx.lib)
        self.ctx, self.nstreams = ctx, nstreams
        check(ctx.lib.sdrhip_fecbuf_create(ctx.h, nstreams, C.byref(self.h)))

    def reset(self, streams=None):
        """constructor state: every stream (sdrhip_fecbuf_reset), or the streams listed (sdrhip_fecbuf_reset_streams: on the
        device, no synchronisation, the others collect on)"""
        if streams is None:
            check(self.ctx.lib.sdrhip_fecbuf_reset(self.h))
        else:
            check(self.ctx.lib.sdrhip_fecbuf_reset_streams(self.h, _stream_mask(streams, self.nstreams)))

    def _read(self, entry, buf, batch_args, max_frames):
        """the tail of both entries: room for max_frames frames per stream, the call -- entry(handle, buf, *batch_args, outputs) --
        and per stream the frames it released"""
        S, F, pb = self.nstreams, max(max_frames, 1), 127 * BLOCK_BYTES
        is_t = _is_torch(buf)
        if is_t:
            data = torch.empty((S, F, pb), dtype=torch.uint8, device=buf.device)
            b0 = torch.empty((S, F, BLOCK_BYTES), dtype=torch.uint8, device=buf.device)
        else:
            data = np.empty((S, F, pb), np.uint8)
            b0 = np.empty((S, F, BLOCK_BYTES), np.uint8)
        info = (FECBufferFrame * (S * F))()
        nf = (C.c_size_t * S)()
        rc = entry(self.h, _ptr(buf), *batch_args, _ptr(data), F * pb, _ptr(b0), max_frames, info, nf, MEM_DEVICE if is_t else MEM_HOST)
        self.last_n_frames = [int(x) for x in nf]
        check(rc)
        return [(data[s, :len(recs)], b0[s, :len(recs)], recs) for s, recs in enumerate(_records(info, F, nf))]

    def write_and_read(self, dgrams_per_stream, max_frames=None):
        S = self.nstreams
        if len(dgrams_per_stream) != S:
            raise ValueError("one datagram array per stream")
        buf, counts, _ = _datagram_batch(dgrams_per_stream)
        if max_frames is None:
            max_frames = max(counts + [0])  # (a call releases at most one frame per datagram)
        return self._read(self.ctx.lib.sdrhip_fecbuf_write_and_read, buf, ((C.c_size_t * S)(*counts), buf.shape[1] * UDPSIZE), max_frames)

    def write_and_read_tagged(self, dgrams, stream_of, max_frames=None):
        """write_and_read of an arrival-order array (sdrhip_fecbuf_write_and_read_tagged): dgrams (n, 512) uint8 -- numpy or a torch
        device tensor --, stream_of (n,) uint16 = the stream of every datagram or DGRAM_SKIP.  Returns what write_and_read returns
        for the per-stream subsequences."""
        buf, tags, tp = _tagged_batch(dgrams, stream_of, allow_torch=True)
        if max_frames is None:  # (a call releases at most one frame per datagram)
            max_frames = int(np.bincount(tags[tags != DGRAM_SKIP], minlength=1).max()) if tags.size else 0
        return self._read(self.ctx.lib.sdrhip_fecbuf_write_and_read_tagged, buf, (tp, buf.shape[0]), max_frames)

    def stats(self, stream):
        """getCurNbBlocks, getCurNbRecovery, getMinNbBlocks, getMaxNbRecovery (these two reset when read), getCurrentMeta,
        getOutputMeta (24 bytes: the 20-byte MetaDataFEC, zero padded) of one stream, as a dict"""
        return _fecbuf_stats(self.ctx, self.h, stream)


def _tagged_batch(dgrams, stream_of, allow_torch=False):
    """an arrival-order array and its tags as the tagged entries take them: (n, 512) uint8 (numpy, used where it lies when it is
    contiguous; a torch device tensor only for the bank), (n,) uint16 numpy tags (SDRHIP_DGRAM_SKIP = 0xffff: no stream)"""
    if _is_torch(dgrams):
        if not allow_torch:
            raise TypeError("submit_datagrams_tagged takes host memory")
        buf = dgrams.reshape(-1, UDPSIZE).contiguous()
        if buf.dtype != torch.uint8:
            raise TypeError("datagrams must be uint8")
    else:
        buf = np.ascontiguousarray(np.asarray(dgrams, np.uint8).reshape(-1, UDPSIZE))
    tags = np.ascontiguousarray(np.asarray(stream_of).reshape(-1), np.uint16)
    if tags.shape[0] != buf.shape[0]:
        raise ValueError("one tag per datagram")
    return buf, tags, tags.ctypes.data_as(C.POINTER(C.c_uint16))


def _datagram_batch(dgrams_per_stream):
    """one (n_s, 512) uint8 array per stream -> (S, max n_s, 512) batch (torch on the device when any input is a torch tensor,
    else numpy), the counts, is_torch"""
    S = len(dgrams_per_stream)
    is_t = any(_is_torch(d) for d in dgrams_per_stream)
    counts = [int(d.shape[0]) for d in dgrams_per_stream]
    nmax = max(counts + [0])
    if is_t:
        dev = next(d.device for d in dgrams_per_stream if _is_torch(d))
        buf = torch.zeros((S, max(nmax, 1), UDPSIZE), dtype=torch.uint8, device=dev)
        for s, d in enumerate(dgrams_per_stream):
            if counts[s]:
                buf[s, :counts[s]] = d.reshape(counts[s], UDPSIZE)
    else:
        buf = np.zeros((S, max(nmax, 1), UDPSIZE), np.uint8)
        for s, d in enumerate(dgrams_per_stream):
            if counts[s]:
                buf[s, :counts[s]] = np.asarray(d, np.uint8).reshape(counts[s], UDPSIZE)
    return buf, counts, is_t


def _fecbuf_stats(ctx, h, stream):
    v = [C.c_int() for _ in range(4)]
    cm, om = (C.c_uint8 * 24)(), (C.c_uint8 * 24)()
    check(ctx.lib.sdrhip_fecbuf_stats(h, stream, *[C.byref(x) for x in v], cm, om))
    return dict(cur_nb_blocks=v[0].value, cur_nb_recovery=v[1].value, min_nb_blocks=v[2].value, max_nb_recovery=v[3].value,
                current_meta=bytes(cm), output_meta=bytes(om))
