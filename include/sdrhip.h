/*
 * sdrhip.h -- C ABI of libsdrhip.so: the MI355X (gfx950) engine behind sdrdaemon's
 * data-parallel hot path (integer half-band decimators / interpolators and the CM256
 * Cauchy-MDS GF(256) block-erasure code).
 *
 * This is the drop-in boundary.  Every entry point states the reference interface it
 * replaces (file:line relative to the f4exb/sdrdaemon tree).  Plain pointers and sizes
 * only; no C++ or torch types.  All functions return 0 on success or a negative
 * SDRHIP_E* code; sdrhip_last_error() gives the message of the calling thread's last
 * failure.
 *
 * Threading: every entry point takes its context's (recursive) lock, so calls on the handles
 * of one context serialise and may come from any thread; handles of different contexts run
 * concurrently (objects that live on different threads in the reference own a context each).
 * Memory: every data pointer is either host memory (SDRHIP_MEM_HOST: the library
 * stages it through pinned buffers and copies back, synchronously) or device memory on
 * the context's GPU (SDRHIP_MEM_DEVICE: 16-byte aligned, work is enqueued on the
 * context's HIP stream and NOT synchronised -- call sdrhip_ctx_synchronize()).
 * IQ samples are interleaved little-endian {int16 re, int16 im} = IQSample
 * (SDRDaemon.h:52-70); sample counts are in IQ samples, not int16 words.
 */
#ifndef SDRHIP_H
#define SDRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRHIP_OK 0
#define SDRHIP_EINVAL (-1)   /* bad argument */
#define SDRHIP_ENOMEM (-2)   /* host or device allocation failed */
#define SDRHIP_EDEVICE (-3)  /* HIP runtime error (no GPU, launch failure ...) */
#define SDRHIP_EALIGN (-4)   /* device pointer / stride not 16-byte aligned */
#define SDRHIP_EDECODE (-5)  /* cm256 decode: duplicate original index / singular system */
#define SDRHIP_EBUSY (-6)    /* asynchronous entry: nothing to collect yet / every batch of the ring is in flight */

#define SDRHIP_MEM_HOST 0
#define SDRHIP_MEM_DEVICE 1

/* Downsampler::fcPos_t, Downsampler.h:29-33 */
#define SDRHIP_FC_INF 0
#define SDRHIP_FC_SUP 1
#define SDRHIP_FC_CEN 2

/* IntHalfbandFilterEO1 (x86 USE_SSE4_1 builds, centre tap x << 13, EO1.h:136-142) versus
 * IntHalfbandFilterDB (all other builds, (x + 1) << 13, DB.h:102-103): Decimators.h:24-28 */
#define SDRHIP_HB_EO1 0
#define SDRHIP_HB_DB 1

/* frame geometry, UDPSinkFEC.h:56-59,109 */
#define SDRHIP_UDPSIZE 512
#define SDRHIP_NB_ORIGINAL 128
#define SDRHIP_BLOCK_BYTES 508
#define SDRHIP_SAMPLES_PER_BLOCK 127
#define SDRHIP_SAMPLES_PER_FRAME 16129

const char *sdrhip_last_error(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int sdrhip_device_count(void);

/* ------------------------------------------------------------------ context -- */
/* One per GPU and host thread of control.  hip_stream: a hipStream_t to enqueue on
 * (e.g. torch.cuda.current_stream().cuda_stream), or NULL for the device's null stream. */
typedef struct sdrhip_ctx sdrhip_ctx;
int sdrhip_ctx_create(int device, void *hip_stream, sdrhip_ctx **out);
/* Handles created on a context keep it alive: destroying the context first only marks it, the last
 * handle to be destroyed frees it. */
void sdrhip_ctx_destroy(sdrhip_ctx *ctx);
int sdrhip_ctx_synchronize(sdrhip_ctx *ctx);
/* Kernel-path knobs for tests and tools (production code never needs them).  The defaults are read from the environment
 * ONCE, when the context is created (SDRHIP_DECIM_PATH, SDRHIP_MFMA_SPAN, SDRHIP_MFMA_MIN, SDRHIP_INTERP_PATH,
 * SDRHIP_INTERP_SPAN, SDRHIP_RX_FUSED, SDRHIP_RX_DIRECT, SDRHIP_RX_WINDOW, SDRHIP_ENC_PATH, SDRHIP_ENC_MIN_ROWS, SDRHIP_MFMA_RING,
 * SDRHIP_TX_OVERLAP, SDRHIP_DEC_PATH, SDRHIP_DEC_PLAN, SDRHIP_FEC_STAGGER[_MOD]); keys:
 * "decim_path" = auto | valu | mfma, "mfma_span" / "mfma_min" / "interp_span" = decimal sample counts, "interp_path" = auto | wave | valu
 * (wave = K5w, the default from interpolate4 up; valu = K5), "rx_fused" = 0 | 1 | 2 | overlap (pipelined Rx: where the deferred encode
 * runs), "rx_direct" = 1 | 0 (Rx pipe on the matrix-core decimator: frame-layout stores, the default, or stream order + framing pass),
 * "enc_path" = fft | karatsuba (CM256 128 + R encoder and the batched decoder's walk: additive FFT for R <= 32, the default, or the
 * Karatsuba XOR-convolution walk), "enc_min_rows" = 1..32 (fewest recovery blocks the FFT encoder serves; below: the generic matrix
 * kernel), "enc_units" = frame | half (the FFT encoder's workgroup: a frame, the default, or one column half of a frame -- an experiment, no faster), "enc_form" = bitslice | table (the FFT encoder in whole-frame
 * workgroups: inverse stages 3..5, the folds and the first forward stage as compile-time XOR trees on bit planes, the default, or every
 * multiplication through the lookup tables; enc_units = half always runs the table form), "mfma_ring" = 4 | 3 | 2 (2: the two-waves-per-SIMD experiment, slower), "tx_overlap" = 1 | 0 (pipelined Tx: decode on the second stream), "dec_path" = syndrome | dense, "dec_plan" =
 * fused | kernel (batched decode with dec_max_rows <= 32 on the FFT decoder: each frame's plan is made by the decoder's own
 * workgroup, the default, or by the planning kernel in a launch of its own), "rx_window" = 0 | 1..8 (frame window of the Rx pipe in
 * calls; 0 = the default: 2, pipelined pipes 4), "fec_stagger" / "fec_stagger_mod" (experiment: staggered start of the FFT encoder's /
 * decoder's workgroups, default off; mod 0: phase = resident round, 1..16: workgroup mod m, 100 + m: the workgroup's arrival rank on its CU mod m), "ktime_stride" = 1..1024 / "ktime_stride_class" = "<class>:<stride>" (the kernel-class timers
 * of sdrhip_ctx_kernel_timing bracket every n-th launch, of all classes / of one).  Every setting computes the same bytes.  One knob is a promise, not a path: "dec_max_rows" = 1..128 | auto (default 128).  A number is the most recovery
 * blocks a received frame can carry AND bounds their row indices: it is the sender's fecblk (known from the meta block), every
 * recovery block of every frame has a row below it -- not a count of the recovery blocks that happened to arrive (a fecblk-64
 * sender's frame can hold five of them and a row of 40); <= 32 makes the batched decode ONE launch (the plan inside the
 * decoder, no fallback kernel).  The count is checked on the device: a frame that carries MORE recovery blocks than
 * dec_max_rows is left as received (like an undecodable frame: missing originals read zero) and counted, see
 * sdrhip_ctx_get_counter("dec_rows_exceeded"); the rows are the caller's word.  "auto" is a mode, not a promise: the library
 * decides per frame from the frame's own block indices (header byte 2, or the `indices` array when one is given).  With N the number of
 * indices >= 128 among the frame's 128 received blocks and maxrow the highest of them minus 128, a frame is DEFERRED iff N > 32 or
 * maxrow >= 32 (whatever else is true of it), every other frame is served by the one-launch decoder exactly as under dec_max_rows =
 * 32; the deferred frames are listed on the device and decoded by the launches behind it exactly as under dec_max_rows = 128 (no
 * host read-back in between), and counted in sdrhip_ctx_get_counter("dec_deferred").  Under auto every batch -- dec_strict 0 or 1, header
 * indices or the `indices` array -- is delivered byte for byte as under dec_max_rows = 128, and "dec_rows_exceeded" does not grow.
 * Where the one-launch decoder is not in play (dec_plan = kernel, dec_path = dense, enc_path = karatsuba) auto reads as 128 and
 * defers nothing; "tx_gather" keeps requiring a number <= 32.  One knob selects behaviour: "dec_strict" = 0 | 1 (default 0).  The reference copies
 * back only the descriptors [128 - recoveryCount, 128) after cm256_decode (SDRdaemonFECBuffer.cpp:204-211: it relies on the
 * recovery blocks arriving last), so a block restored into a recovery block that arrived BEFORE some original is never copied
 * and stays a hole; by default the batched decoder delivers every restored block (a superset), with dec_strict = 1 exactly the
 * reference's frames, holes included. */
int sdrhip_ctx_set_option(sdrhip_ctx *ctx, const char *key, const char *value);
/* Event counters of the context.  Keys:
 * "dec_rows_exceeded" = frames, since the context was created, that the batched decoder (sdrhip_fec_decode_frames,
 * sdrhip_tx_process) left unrepaired because they carried more recovery blocks than the dec_max_rows option allows (kept on the
 * device: reading it synchronises the context's stream); it does not grow under dec_max_rows = auto;
 * "dec_deferred" = frames, since the context was created, that the one-launch decoder handed to the launches behind it under
 * dec_max_rows = auto (more than 32 recovery blocks, or a recovery row >= 32, among the frame's 128 blocks; on the device, as above);
 * "fecbuf_shadow_mismatch" = streams of asynchronous datagram batches of either pipe (sdrhip_tx_submit_datagrams,
 * sdrhip_rx_submit_datagrams) whose collector counts on the
 * device disagreed with the host's shadow that sized the batch's grids; 0 unless the library is broken (on the device, as above);
 * "h2d_bytes" / "d2h_bytes" = bytes that the context's entry points have copied from host to device / device to host since the
 * context was created (staging copies of host-memory calls, including the kernels' direct reads of pinned staging memory for
 * small calls; not the constant tables of sdrhip_ctx_create).  Counted on the host when the copy is enqueued: reading them does
 * not synchronise. */
int sdrhip_ctx_get_counter(sdrhip_ctx *ctx, const char *key, uint64_t *value);
/* Average duration in milliseconds of the kernels launched between timing_begin and
 * timing_end on the context's stream, measured with hipEvents on that stream (what
 * bench.py's roofline object reports). */
int sdrhip_ctx_timing_begin(sdrhip_ctx *ctx);
int sdrhip_ctx_timing_end(sdrhip_ctx *ctx, float *elapsed_ms);
/* Per-kernel-class timing: while enabled, every launch of the class is bracketed by
 * hipEvents on the context's stream.  _read synchronises, returns the summed duration and
 * the number of launches since the last read, and clears the log.  An event pair costs the
 * stream ~2.5 us: sdrhip_ctx_set_option("ktime_stride", "N") brackets only every N-th launch of
 * a class (default 1; bench.py samples every 4th step of its timed region).  Classes: */
#define SDRHIP_K_DECIMATE 0    /* half-band decimator cascade kernel */
#define SDRHIP_K_INTERPOLATE 1 /* half-band interpolator cascade kernel */
#define SDRHIP_K_FEC_ENCODE 2  /* GF(256) matrix apply, encoder rows */
#define SDRHIP_K_FEC_DECODE 3  /* GF(256) matrix apply, decode matrices */
#define SDRHIP_K_CONVERT 4     /* 8-bit IQ widening pass of the Rx pipe (sdrhip_rx_set_input_format) */
int sdrhip_ctx_kernel_timing(sdrhip_ctx *ctx, int enable);
int sdrhip_ctx_kernel_timing_read(sdrhip_ctx *ctx, int kernel_class, double *total_ms, unsigned *launches);

/* --------------------------------------------------------------- decimators -- */
/* A bank of `nstreams` independent `Decimators` objects (Decimators.h:32-71): per stream
 * the six half-band filter states m_decimator2..64 persist across calls, exactly like the
 * reference members.  hb_variant selects EO1 / DB rounding. */
typedef struct sdrhip_decimators sdrhip_decimators;
int sdrhip_decimators_create(sdrhip_ctx *ctx, int nstreams, int hb_variant, sdrhip_decimators **out);
void sdrhip_decimators_destroy(sdrhip_decimators *d);
int sdrhip_decimators_reset(sdrhip_decimators *d); /* back to the constructor's zero state */
/* What the bank's last cascade launch was (diagnostics: bench.py labels its roofline kernel with it, the parity tests
 * assert that they ran the benchmarked geometry).  path: 0 = the last call launched no cascade kernel (none yet, an empty call,
 * decimate1 and the filter-less decimate2 / 4_inf / _sup), 1 = VALU kernel (nseg segments per
 * stream), 2 = matrix-core kernel (per stream: VALU head [0, head), wps waves x 8 spans of `span` samples, VALU tail from
 * tail_start in npieces - 1 pieces). */
typedef struct sdrhip_decim_plan {
    int path, wps, npieces, nseg;
    size_t span, head, tail_start;
} sdrhip_decim_plan;
int sdrhip_decimators_last_plan(const sdrhip_decimators *d, sdrhip_decim_plan *out);

/* One Decimators::decimate<2^log2decim>_{inf,sup,cen}(sampleSize, in, out) call
 * (Decimators.h:35-53; dispatch of Downsampler::process, Downsampler.cpp:74-162) on each
 * stream of the bank.  log2decim 0..6 (0 = Downsampler's copy + decimate1 rescale,
 * Decimators.cpp:22-35), fcpos SDRHIP_FC_*.  Stream s reads n_in samples at
 * iq_in + 2*s*in_stride and writes *n_out = n_in >> log2decim samples (what the reference
 * resizes `out` to) at iq_out + 2*s*out_stride (strides in samples; ignored for one
 * stream).  *sampleSize (effective bits, 8..16) is updated as the reference's by-reference
 * argument.  As in the reference, floor(n_in / N) * N samples are consumed and the
 * remainder never enters the filter history.  No byte of row s past *n_out samples is
 * written -- not the gap up to out_stride, nothing in front of the first or behind the
 * last row --, the input is only read, and neither the result nor the state the call
 * leaves depends on memory behind n_in samples of a row (the dropped remainder
 * included), in host and in device memory (tests/test_gpu_bank_bounds.py). */
int sdrhip_decimate(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                    size_t n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* Decimators bank, ragged: stream s consumes n_in[s] samples (remainder below 2^log2decim dropped per stream, as
 * sdrhip_decimate drops it for all); n_out[s] = n_in[s] >> log2decim. in_stride / out_stride >= the largest count.
 * n_in and n_out are host arrays of nstreams entries.  A stream with n_in[s] < 2^log2decim keeps its filter history as it was.
 * Host memory: only n_in[s] samples of row s are read and n_out[s] written.  Device memory: the alignment rules of
 * sdrhip_decimate; the kernels read no sample of stream s past n_in[s] (the last row may be exactly n_in[nstreams - 1] long).
 * One launch serves every stream, chosen as for sdrhip_decimate (context option decim_path, mfma_min of the call's total samples):
 * the matrix-core cascade with per-stream wave groups and pieces (sdrhip_decimators_last_plan: path 2, span / head shared, wps /
 * npieces = the launch's totals) or the VALU cascade with a per-call work table (path 1, nseg = the launch's workgroups).
 * *sampleSize advances as in sdrhip_decimate. */
int sdrhip_decimate_ragged(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                           const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* sdrhip_decimate_ragged with sampleSize an ARRAY of nstreams entries (each 1..16), read and advanced per stream: in the
 * reference every sdrdaemonrx process hands its own source's get_sample_bits() to Downsampler::process (sdrdaemonrx.cpp:619-620,
 * 639-640; RtlSdrSource.cpp:549 and HackRFSource.cpp:669 say 8), and the size enters a cascade in one place only, the final
 * `x << norm_shift >> trunk_shift` in front of the int16 truncation (Decimators.cpp:27-32, 43-44, 52-53, 62 and every decimateN).
 * Stream s gets the samples of a one-stream bank called with sampleSize[s]; the same launch as sdrhip_decimate_ragged serves the
 * call (each stream's shift pair travels in its row of the per-call table).  Everything else as sdrhip_decimate_ragged. */
int sdrhip_decimate_ragged_bits(sdrhip_decimators *d, int log2decim, int fcpos, unsigned *sampleSize, const int16_t *iq_in,
                                const size_t *n_in, size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* Decimators bank, taps: every rate of a centred cascade in one launch -- one radio head served to several clients at /4, /16 and
 * /64 reads its samples once and runs the shared stages once.  The reference's centred cascades nest (Decimators.h:38-53):
 * decimate4_cen is m_decimator2 -> m_decimator4 (Decimators.cpp:173-213), decimate16_cen the same two stages and two more
 * (Decimators.cpp:403-516), decimate64_cen those four and two more (Decimators.cpp:902-1305); decimate2_cen (Decimators.cpp:94-120)
 * is the first stage alone.  Every stage is the same HB64 filter, the stages hand each other unshifted int32, and sampleSize enters
 * in one place only, the final `x << norm_shift >> trunk_shift`.  So stage k of a longer cascade, shifted for decimate<2^k>_cen,
 * IS that cascade's output (Downsampler::process dispatches to them, Downsampler.cpp:74-162).
 * tap_mask: bit k set (k = 1..6) = a tap at /2^k; L = the highest set bit.  Bit 0, bits above 6 and an empty mask are refused.
 * n_in: host array of nstreams counts, which may differ and may be 0.  n_used[s] = (n_in[s] >> L) << L is returned in the host
 * array n_used; tap k of stream s receives n_used[s] >> k samples at taps->iq_out[k] + 2 * s * taps->out_stride[k], and
 * taps->sample_size[k] the by-reference sampleSize after decimate<2^k>_cen (slots of taps that are not set are neither read nor
 * written).  For every set k and every stream the samples and sample_size[k] are byte for byte those of a reference Decimators
 * object of its own (one-stream EO1 or DB, as the bank) that calls decimate<2^k>_cen(sampleSize, x[0 : n_used[s]]) and continues
 * from call to call.  The bank's state afterwards is byte for byte that of sdrhip_decimate_ragged(d, L, SDRHIP_FC_CEN, ...) on the
 * same counts: the entry mixes freely with sdrhip_decimate, _ragged and _ragged_bits on one bank; a stream with n_in[s] < 2^L keeps
 * its histories exactly; a call whose counts are all below 2^L launches nothing (sdrhip_decimators_last_plan: path 0).
 * One launch serves every stream and every tap: the VALU cascade with the per-call work table of sdrhip_decimate_ragged and a
 * store per tapped stage (sdrhip_decimators_last_plan: path 1, nseg = the launch's workgroups), whatever decim_path says -- the
 * matrix-core kernel does not serve this entry.  A mask with one bit set launches the existing kernels, as sdrhip_decimate_ragged
 * picks them.
 * Device memory: the alignment rules of sdrhip_decimate for iq_in and every tapped iq_out[k] / out_stride[k] (pointers 16-byte
 * aligned, strides multiples of 4 samples); out_stride[k] >= max_s n_used[s] >> k, in_stride >= max n_in.  No byte of a tap's row
 * past its count is written, and nothing between or around rows; no sample of stream s behind n_in[s] is read, and nothing depends
 * on the dropped remainder.  Host memory: the samples go up once, exactly 4 * sum_s n_in[s] bytes ("h2d_bytes"), the results come
 * down as exactly 4 * sum_k sum_s (n_used[s] >> k) bytes ("d2h_bytes"), only those samples of the caller's rows are written, and
 * the call returns with the outputs written (a call that launches nothing moves nothing).
 * SDRHIP_EINVAL, with nothing consumed, enqueued or changed: a NULL handle, taps, n_in or n_used; a bad mask; sampleSize outside
 * 1..16; a NULL buffer of a tapped slot, or a NULL input, while any stream has output; a stride below its largest count; more
 * segments than a grid holds.  Broken alignment: SDRHIP_EALIGN, likewise with nothing consumed.
 * Not covered: the inf / sup cascades (they nest from /8 on), a per-stream sampleSize, the matrix-core path, taps inside sdrhip_rx
 * itself (a fan-out hub composes this entry with one sdrhip_rx bank: INTEGRATION.md), the C++ adapter headers, tools/fuzz_gpu.py. */
#define SDRHIP_DECIM_TAP_SLOTS 7   /* index k = log2 of a tap's decimation; slot 0 is not used */
typedef struct sdrhip_decim_taps {
    int16_t *iq_out[SDRHIP_DECIM_TAP_SLOTS];      /* tap k, stream s: iq_out[k] + 2 * s * out_stride[k] */
    size_t out_stride[SDRHIP_DECIM_TAP_SLOTS];    /* samples; ignored for one stream */
    unsigned sample_size[SDRHIP_DECIM_TAP_SLOTS]; /* out: the by-reference sampleSize after decimate<2^k>_cen */
} sdrhip_decim_taps;
int sdrhip_decimate_taps(sdrhip_decimators *d, unsigned tap_mask, unsigned sampleSize, const int16_t *iq_in,
                         const size_t *n_in, size_t in_stride, sdrhip_decim_taps *taps, size_t *n_used, int mem);

/* ------------------------------------------------------------ interpolators -- */
/* Bank of `Interpolators` objects (Interpolators.h:35-61): HB64, HB32, 4 x HB16 states. */
typedef struct sdrhip_interpolators sdrhip_interpolators;
int sdrhip_interpolators_create(sdrhip_ctx *ctx, int nstreams, sdrhip_interpolators **out);
void sdrhip_interpolators_destroy(sdrhip_interpolators *p);
int sdrhip_interpolators_reset(sdrhip_interpolators *p);
/* One Interpolators::interpolate<2^log2interp>_cen(in, out) call per stream
 * (Interpolators.h:38-43; Upsampler::process, Upsampler.cpp:52-84; log2interp 0 copies).
 * *n_out = n_in << log2interp.  log2interp = 6 reproduces the reference's
 * interpolate64_cen as it is (32 interpolated + 32 zero samples per input,
 * Interpolators.cpp:363-606).  Stream s reads n_in samples at iq_in + 2*s*in_stride and
 * writes *n_out at iq_out + 2*s*out_stride (strides in samples; ignored for one stream).
 * No byte of row s past *n_out samples is written, the input is only read, and neither
 * the result nor the state the call leaves depends on memory behind n_in samples of a
 * row, in host and in device memory (tests/test_gpu_bank_bounds.py). */
int sdrhip_interpolate(sdrhip_interpolators *p, int log2interp, const int16_t *iq_in, size_t n_in,
                       size_t in_stride, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* Interpolators bank, ragged: one Interpolators::interpolate<2^log2interp>_cen call per stream (Interpolators.h:38-43;
 * Upsampler::process, Upsampler.cpp:52-84; Interpolators.cpp:363-606 for log2interp = 6, as sdrhip_interpolate has it) in which
 * stream s consumes n_in[s] samples at iq_in + 2*s*in_stride and writes n_out[s] = n_in[s] << log2interp samples at
 * iq_out + 2*s*out_stride.  n_in and n_out are host arrays of nstreams entries; in_stride >= the largest n_in[s], out_stride >=
 * the largest n_out[s] (strides in samples; ignored for one stream).  log2interp 0..6 (0 copies n_in[s] samples per row).
 * Per stream, the output and the bank's state afterwards are byte for byte those of a one-stream bank given the same chunks in
 * the same order: any count is legal, 0, 1 and odd ones included, and a stream with n_in[s] == 0 keeps its six filter histories
 * exactly.  A call whose counts are all 0 launches nothing.  The entry mixes freely with sdrhip_interpolate on one bank.
 * One launch serves every stream (K5c): the kernels of sdrhip_interpolate (context options interp_path, interp_span) on a compact
 * grid, one workgroup (or one wave of a workgroup) per (stream, segment) of a per-call table, sum_s max(1, ceil(n_in[s] / segment))
 * entries, with one segment length for the launch, taken from the largest count as sdrhip_interpolate takes it from n_in:
 * the launch's cost follows the samples, not nstreams x the largest count (sdrhip_interpolators_last_plan: compact = 1).
 * Host memory: only n_in[s] samples of row s are read and only n_out[s] written; the samples go up in one packed copy of exactly
 * 4 * sum_s n_in[s] bytes and the results come down in one packed copy of exactly 4 * sum_s n_out[s] bytes ("h2d_bytes" /
 * "d2h_bytes"; log2interp = 1 alone rounds every stream's share of the download up to 16 bytes).
 * Device memory: the alignment rules of sdrhip_interpolate (pointers 16-byte aligned, strides multiples of 4 samples for more
 * than one stream).  No byte of row s past n_out[s] samples is written, and the kernels read no sample of stream s past n_in[s]
 * (every load of either kernel is guarded by the stream's own end; the last row may be exactly n_in[nstreams - 1] long).
 * Refused with SDRHIP_EINVAL and nothing consumed, enqueued or changed: a NULL handle, NULL n_in or n_out, a NULL buffer with any
 * count non-zero, a stride below the largest count, a count of 2^31 samples or more, more than 2^31 - 1 table entries (the grid).
 * Device pointers or strides that break the alignment rules: SDRHIP_EALIGN, likewise nothing consumed. */
int sdrhip_interpolate_ragged(sdrhip_interpolators *p, int log2interp, const int16_t *iq_in, const size_t *n_in, size_t in_stride,
                              int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* What the bank's last launch was (diagnostics, as sdrhip_decimators_last_plan).  path: 0 = the last call launched nothing (none
 * yet, an empty or a refused-by-the-device call), SDRHIP_INTERP_COPY = the x1 copy, SDRHIP_INTERP_VALU = K5 (workgroups of 256
 * lanes, segments of whole macro-cycles), SDRHIP_INTERP_WAVE = K5w (wave-private pipelines, segments of 128-input blocks).
 * seg_len = the segment length in inputs, wpw = waves per workgroup of K5w (1 or 4; 1 elsewhere), entries = the (stream, segment)
 * pairs the launch served, compact = 1 for sdrhip_interpolate_ragged's grid (one entry per pair that exists), 0 for the
 * rectangular grids of sdrhip_interpolate and the Tx pipe (entries = segments of the longest stream x nstreams; the x1 copy
 * reports nstreams entries of n_in samples). */
#define SDRHIP_INTERP_COPY 1
#define SDRHIP_INTERP_VALU 2
#define SDRHIP_INTERP_WAVE 3
typedef struct sdrhip_interp_plan {
    int path, wpw, compact, reserved;
    size_t seg_len, entries;
} sdrhip_interp_plan;
int sdrhip_interpolators_last_plan(const sdrhip_interpolators *p, sdrhip_interp_plan *out);

/* -------------------------------------------------------------------- CM256 -- */
/* CM256::cm256_encoder_params / CM256::cm256_block as used at UDPSinkFEC.cpp:195-246 and
 * SDRdaemonFECBuffer.cpp:148-197 (layout-compatible with cm256cc's structs). */
typedef struct {
    int OriginalCount;
    int RecoveryCount;
    int BlockBytes;
} sdrhip_cm256_params;
typedef struct {
    void *Block;
    unsigned char Index;
} sdrhip_cm256_block;

/* CM256::cm256_encode(params, originals, recoveryBlocks) (UDPSinkFEC.cpp:246): host
 * pointers; originals taken positionally; recovery block r is Cauchy row OriginalCount + r. */
int sdrhip_cm256_encode(sdrhip_ctx *ctx, sdrhip_cm256_params params, const sdrhip_cm256_block *originals,
                        void *recoveryBlocks);
/* CM256::cm256_decode(params, blocks) (SDRdaemonFECBuffer.cpp:197): host pointers, in-place
 * contract of the library: recovered originals overwrite the recovery blocks' buffers and
 * their Index becomes the recovered original's index.  RecoveryCount == 1 takes the
 * library's XOR shortcut (see DESIGN.md "mirrored quirks"). */
int sdrhip_cm256_decode(sdrhip_ctx *ctx, sdrhip_cm256_params params, sdrhip_cm256_block *blocks);

/* Batched form of the encode section of UDPSinkFEC::transmitUDP (UDPSinkFEC.cpp:228-256):
 * frames = nframes x 128 super blocks of 512 bytes (header + 508 protected bytes);
 * recovery_out = nframes x nb_fec super blocks with header {frameIndex, 128 + r, 0}. */
int sdrhip_fec_encode_frames(sdrhip_ctx *ctx, const uint8_t *frames, size_t nframes, int nb_fec,
                             uint8_t *recovery_out, int mem);
/* Batched form of the decode section of SDRdaemonFECBuffer::writeAndRead
 * (SDRdaemonFECBuffer.cpp:143-213) + getSlotData (:72-75): rx = nframes x 128 super
 * blocks, the first 128 datagrams of each frame in arrival order (originals and recovery
 * mixed; the reference relies on recovery blocks arriving last, :210); payload_out =
 * nframes x 127 x 508 bytes (blocks 1..127 in place, i.e. 16129 IQ samples per frame);
 * block0_out (may be NULL) = nframes x 508 bytes (the meta block).  The block indices are
 * header.blockIndex of the super blocks (:147), read on the device; `indices` (may be NULL;
 * nframes x 128 bytes, HOST memory in either mode) overrides them.  Planning (which
 * originals are missing, the inverse of the Cauchy block, the recovery matrix of every
 * frame) runs on the GPU: a batch may hold any number of distinct loss patterns and the
 * device-memory form never synchronises with the host. */
int sdrhip_fec_decode_frames(sdrhip_ctx *ctx, const uint8_t *rx, const uint8_t *indices, size_t nframes,
                             uint8_t *payload_out, uint8_t *block0_out, int mem);

/* ----------------------------------------------------------- TestSource bank -- */
/* A bank of `nstreams` TestSource devices (include/TestSource.h:29-116, sdmnbase/TestSource.cpp) producing their
 * 16-bit IQ samples straight into device memory: the input side of BASELINE configs 2-5 without an H2D copy.
 * Configuration = the reference's key=value string (TestSource.cpp:59-215: srate, freq, dfp, dfn, power, blklen,
 * fcpos, decim; same range checks, same error strings through sdrhip_last_error(), same quirks -- see
 * sdrhip_testsource.cpp).  The sample arithmetic is NOT the reference's float phasor (not reproducible:
 * -ffast-math, wrap bug :411-415) but an integer-exact NCO defined in testsource_kernels.hip and restated in
 * oracle/sdr_oracle.c.  No real-time pacing (the reference sleeps one block time per block, :418). */
typedef struct sdrhip_testsource sdrhip_testsource;
int sdrhip_testsource_create(sdrhip_ctx *ctx, int nstreams, sdrhip_testsource **out);
void sdrhip_testsource_destroy(sdrhip_testsource *ts);
/* TestSource::configure(parsekv::pairs_type&): kv = "key=value,key=value" (',' or '&' separated, parsekv.h:40-43);
 * stream = -1 configures every stream. */
int sdrhip_testsource_configure(sdrhip_testsource *ts, int stream, const char *kv);
/* get_sample_rate() / get_frequency() (TestSource.cpp:261-270), block length, forwarded decim / fcpos; any pointer may be NULL */
int sdrhip_testsource_get(const sdrhip_testsource *ts, int stream, uint32_t *sample_rate, uint32_t *frequency, int *block_length,
                          int *log2decim, int *fcpos);
/* the next n samples of every stream (stream s at iq_out + 2*s*out_stride), phase continuous across calls.  No byte of row s
 * past n samples is written, in host and in device memory (tests/test_gpu_bank_bounds.py). */
int sdrhip_testsource_read(sdrhip_testsource *ts, int16_t *iq_out, size_t n, size_t out_stride, int mem);

/* ---------------------------------------------------------- IQ sample formats -- */
/* What the data entries of an Rx / Tx pipe take or give per IQ sample (sdrhip_rx_set_input_format, sdrhip_tx_set_output_format).
 * The pointer parameters keep their declared types: with an 8-bit format they point at 2-byte samples and the caller casts.
 * Sample counts and strides stay in samples. */
#define SDRHIP_IQ_S16 0 /* IQSample {int16 re, int16 im} (SDRDaemon.h:52-70): every entry's format by default */
#define SDRHIP_IQ_U8 1  /* RTL-SDR: {uint8 re, uint8 im} offset binary, widened to IQSample(b - 128) (RtlSdrSource.cpp:542-553) */
#define SDRHIP_IQ_S8 2  /* HackRF: {int8 re, int8 im}; in: IQSample(b) (HackRFSource.cpp:661-674), out: (int8)(v >> 8)
                         * of each component (HackRFSink.cpp:671-672) */

/* ------------------------------------------------------------ fused Rx pipe -- */
/* Bank of Rx chains: Downsampler::process (Downsampler.cpp:74-162) -> UDPSinkFEC::write
 * framing (UDPSinkFEC.cpp:79-191) -> encode section of transmitUDP (:228-256), i.e. what
 * sdrdaemonrx's main loop + writer + tx threads compute between source_buffer.pull() and
 * sendto() (sdrdaemonrx.cpp:579-663). */
typedef struct {
    int log2decim;                 /* decim=  0..6 */
    int fcpos;                     /* fcpos=  0..2 */
    int hb_variant;                /* SDRHIP_HB_EO1 / SDRHIP_HB_DB */
    unsigned sample_bits;          /* DeviceSource::get_sample_bits(), 8..16 */
    int nb_fec;                    /* fecblk= 0..128 */
    uint32_t center_frequency_khz; /* UDPSink::setCenterFrequency (kHz on the wire, UDPSink.h:93) */
    uint32_t sample_rate;          /* rate AFTER decimation, UDPSink::setSampleRate */
} sdrhip_rx_config;
typedef struct sdrhip_rx sdrhip_rx;
int sdrhip_rx_create(sdrhip_ctx *ctx, int nstreams, const sdrhip_rx_config *cfg, sdrhip_rx **out);
void sdrhip_rx_destroy(sdrhip_rx *rx);
/* Live reconfiguration between two sdrhip_rx_process calls, the way sdrdaemonrx applies a control
 * message (Downsampler::configure, Downsampler.cpp:32-67: decim / fcpos; UDPSink::setNbBlocksFEC,
 * setCenterFrequency, setSampleRate, sdrdaemonrx.cpp:300-340).  As in the reference the filter
 * states carry over (the six half-band instances are shared by every decimateN entry point), the
 * frame being filled keeps the meta block it was started with and is encoded with the fecblk value
 * in force when it completes (UDPSinkFEC.cpp:160-165).  hb_variant cannot change. */
int sdrhip_rx_reconfigure(sdrhip_rx *rx, const sdrhip_rx_config *cfg);
/* Per-stream UDPSink::setCenterFrequency / setSampleRate (UDPSink.h:93-96; sdrdaemonrx.cpp:597,624,644: every sdrdaemonrx sets them
 * from its own source).  Host arrays of nstreams entries; NULL = that field is bank-wide again (sdrhip_rx_config's value).
 * A frame of stream s takes, when it is opened: center_frequency_khz[s] and sample_rate[s] in bytes 0..7 of its meta block
 * (UDPSinkFEC.cpp:97-98), the CRC-32 over its own 20 bytes, and a time stamp advanced by ITS OWN sample clock: floor(p * 10^6 /
 * sample_rate[s]) microseconds for a frame that starts p decimated samples into the call (sample_rate[s] = 0: no advance).  Per
 * stream the result is byte for byte that of a one-stream sdrhip_rx whose config carries that stream's two values -- meta block and
 * the recovery blocks computed over it -- through every entry: sdrhip_rx_process (immediate and pipelined, sdrhip_rx_flush),
 * sdrhip_rx_process_ragged, sdrhip_rx_submit / _collect, sdrhip_rx_submit_ragged / _collect_ragged, sdrhip_rx_process_datagrams
 * and sdrhip_rx_submit_datagrams / _collect_datagrams.
 * While an array is set for a field, the config's value of that field is unused; sdrhip_rx_reconfigure does not clear the arrays.
 * sample_rate stays "the rate AFTER decimation", the caller's business as in the config.
 * Allowed at any time, never synchronises: it applies to frames opened by later launches.  A batch takes the values at the moment
 * it takes its sdrhip_rx_config: a datagram batch at submit, a uniform or ragged batch when it is launched.  The frame being filled
 * keeps the meta block it was started with (UDPSinkFEC.cpp:160-165), batches in flight keep theirs, and frames a pipelined call
 * left for the next launch keep the values of the call that opened them.  A handle on which this was never called launches what it
 * launched before the call existed.  SDRHIP_EINVAL, nothing changed: a NULL handle. */
int sdrhip_rx_set_stream_meta(sdrhip_rx *rx, const uint32_t *center_frequency_khz, const uint32_t *sample_rate);
/* what stream s's next opened frame will carry (either pointer may be NULL); SDRHIP_EINVAL: a NULL handle, a stream outside the bank.
 * The host's values: the arrays above, else the config.  Values followed from the incoming meta blocks (sdrhip_rx_set_follow_meta) are
 * never brought to the host: read them from the delivered frames, or through sdrhip_fecbuf_stats on sdrhip_rx_collector. */
int sdrhip_rx_get_stream_meta(const sdrhip_rx *rx, int stream, uint32_t *center_frequency_khz, uint32_t *sample_rate);
/* Outgoing meta from the incoming meta blocks, for the entries fed raw FEC datagrams (sdrhip_rx_process_datagrams,
 * sdrhip_rx_submit_datagrams / _collect_datagrams).  sdrdaemonrx announces the frequency and the rate of its own source
 * (sdrdaemonrx.cpp:622-631,644); a hub's source is the radio head, whose values arrive in the meta block of its frames.  on = 0 is
 * the default.  The call sets a host-side flag only: nothing is enqueued, nothing is waited for.  Allowed at any time: it applies to
 * later sdrhip_rx_process_datagrams calls and later sdrhip_rx_submit_datagrams submits; a batch in flight keeps the mode it was
 * submitted with.  The sample-fed entries (sdrhip_rx_process, _ragged, _submit*) have no incoming meta and ignore the flag.
 * With on != 0, for every datagram call or batch and every stream s:
 *  1. the stream's m_outputMeta is taken as it stands after this call's collection: the state the call commits, what
 *     sdrhip_fecbuf_stats(..., output_meta) reports after the call.  It is the meta block of the last frame released in this or an
 *     earlier call whose block 0 was among its first 128 arrivals (SDRdaemonFECBuffer.cpp:72-85); a frame whose block 0 was lost and
 *     restored by the decoder does not set it (m_metaRetrieved, SDRdaemonFECBuffer.cpp:150-153).
 *  2. m_outputMeta.m_sampleRate != 0: the stream has incoming meta.  Every frame that this call's step opens carries
 *     m_centerFrequency unchanged and m_sampleRate >> log2decim, with the log2decim of the configuration the call or batch runs with
 *     (sdrdaemonrx.cpp:622-631,644).  The shifted rate is also the clock that advances the frame stamps (a shifted rate of 0: every
 *     frame carries the call's stamp), and the CRC is that of the resulting 20-byte record.
 *  3. otherwise (no frame released with its block 0 yet, or a sender that says rate 0) the stream keeps the values it has with the
 *     flag off: the sdrhip_rx_set_stream_meta arrays, else the configuration.
 *  4. a frame left open by an earlier call keeps the block 0 it was opened with (UDPSinkFEC.cpp:160-165).
 *  5. sampleBytes, sampleBits, nbOriginalBlocks, nbFECBlocks and the stamps stay the hub's own: the reference stamps a frame with
 *     gettimeofday where it is opened (UDPSinkFEC.cpp:90-104), so the caller's tv_sec / tv_usec arrays remain right.  (With
 *     sdrhip_rx_set_stream_fec / sdrhip_rx_set_stream_bits arrays "the hub's own" count and sample size are the stream's own.)
 *     sampleBytes and sampleBits stay the hub's own unless sdrhip_rx_set_follow_bits is on: then the record formed here contains the
 *     followed bytes 8 and 9.
 *  6. sdrhip_rx_get_stream_meta keeps reporting the host's values.
 * The values are formed on the device between the collector and the step (one small launch per call or batch); nothing about them
 * comes back to the host, and a submit still synchronises nothing.  With the flag off every entry launches exactly what it launched
 * before the call existed.  SDRHIP_EINVAL, nothing changed: a NULL handle. */
int sdrhip_rx_set_follow_meta(sdrhip_rx *rx, int on);
/* The sample size from the incoming meta blocks, for the same entries (sdrhip_rx_process_datagrams, sdrhip_rx_submit_datagrams[_tagged]
 * / _collect_datagrams, sdrhip_rx_collect_egress): the twin of sdrhip_rx_set_follow_meta for the one value of a stream's signal
 * description that it leaves to the operator.  sdrdaemonrx hands its own source's get_sample_bits() to its Downsampler and,
 * decimated, to its sink (sdrdaemonrx.cpp:619-623, 639-643); a hub's source is the radio head -- 8 for an RTL-SDR or HackRF, 12 for
 * an Airspy or BladeRF, 16 for a test source -- whose size arrives in byte 9 of the meta block of its frames.  on = 0 is the
 * default.  The call sets a host-side flag only: nothing is enqueued, nothing is waited for.  Allowed at any time, also with
 * batches in flight: a datagram call reads the flag per call, a batch at its submit; a batch in flight keeps the mode it was
 * submitted with.  The sample-fed entries (sdrhip_rx_process, _ragged, _submit*) have no incoming meta and ignore the flag.  It is
 * independent of sdrhip_rx_set_follow_meta: either flag, both or neither may be on.
 * With on != 0, for every datagram call or batch and every stream s:
 *  1. the stream's m_outputMeta is taken as it stands after this call's collection, exactly as in rule 1 of
 *     sdrhip_rx_set_follow_meta: the state the call commits, what sdrhip_fecbuf_stats(..., output_meta) reports after the call
 *     (SDRdaemonFECBuffer.cpp:72-85); a block 0 that the decoder restored does not set it (SDRdaemonFECBuffer.cpp:150-153).
 *  2. b = m_outputMeta.m_sampleBits; 1 <= b <= 16: the stream has an incoming size.  Every sample this call's step decimates for the
 *     stream -- the samples held back from earlier calls included: the call is the granularity, as for the rate -- takes the shift
 *     pair of (log2decim, b), `x << norm >> trunk` (Decimators.cpp:27-32, 43-44).  Every frame the step opens carries sampleBits =
 *     b', the size the decimator returns for (log2decim, b), and sampleBytes = (b' - 1) / 8 + 1; the CRC is that of the resulting
 *     record, and the recovery blocks are computed over that block 0.  log2decim is that of the configuration the call or batch
 *     runs with.  Only byte 9 is read: the indicator nibble of the incoming m_sampleBytes is ignored.
 *  3. otherwise (no frame released with its block 0 yet, a sender that says 0, or a value above 16) the stream keeps the size it
 *     has with the flag off: its entry of the sdrhip_rx_set_stream_bits array, else cfg.sample_bits.  With the array set and the
 *     flag on, the followed value wins wherever it exists.
 *  4. a frame left open by an earlier call keeps the block 0 it was opened with (UDPSinkFEC.cpp:160-165); the samples take the new
 *     shift at once: the rule sdrhip_rx_set_stream_bits has for a change of its array.
 *  5. sdrhip_rx_get_stream_bits keeps reporting the host's values: the followed size is never brought to the host.
 *  6. with both flags on, the record sdrhip_rx_set_follow_meta forms (frequency, rate >> log2decim, CRC) contains the followed
 *     bytes 8 and 9.
 *  7. with the flag off, or on a handle where this was never called, every entry launches the kernels it launches today, in the
 *     same order, with the same arguments.
 * sdrhip_rx_reconfigure, sdrhip_rx_export_stream and sdrhip_rx_import_stream leave the flag alone: it is configuration of the
 * handle.  sdrhip_rx_reset_streams resets a stream's collector, which zeroes its m_outputMeta: a reset stream falls back under
 * rule 3 until its head's first block 0 is released.
 * The values are formed on the device between the collector and the step (one small launch per call or batch, in front of the one
 * of sdrhip_rx_set_follow_meta); nothing about them comes back to the host, a submit still synchronises nothing, and the link bytes
 * of a batch are the same with and without the flag.  SDRHIP_EINVAL, nothing changed: a NULL handle. */
int sdrhip_rx_set_follow_bits(sdrhip_rx *rx, int on);
/* Feeds n_in device-rate samples per stream.  Completed frames of stream s are written to
 * frames_out + s*frame_stride_bytes as (128 + nb_fec) super blocks of 512 bytes each,
 * frame after frame; *n_frames (per stream, identical for all streams) is the number of
 * frames completed by this call.  tv_sec/tv_usec = the time of the call's FIRST sample; the
 * meta block of every frame STARTED by this call carries that time advanced by the sample
 * clock to the frame's first sample: + floor(p * 10^6 / sample_rate) microseconds for a frame
 * that starts p decimated samples into the call (sample_rate = the configured rate of the
 * frame stream; 0 = no advance), and the CRC-32 over it (the reference calls gettimeofday
 * when it opens a frame, UDPSinkFEC.cpp:90-115; a batched call opens many at once).
 * frames_out must hold sdrhip_rx_max_frames(rx, n_in) frames per stream. */
int sdrhip_rx_process(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec,
                      uint32_t tv_usec, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames,
                      int mem);
size_t sdrhip_rx_max_frames(const sdrhip_rx *rx, size_t n_in);
/* Pipelined mode (off by default).  The reference's sink is asynchronous as well: UDPSinkFEC::write returns at once and the
 * transmit thread encodes and sends a frame later (UDPSinkFEC.cpp:193-211).  With on != 0 a sdrhip_rx_process call DELIVERS
 * (frames_out, *n_frames, sdrhip_rx_frames_view) the frames that the PREVIOUS call completed; their recovery blocks are computed
 * by encoder workgroups that ride in this call's decimator launch (one launch instead of two, the encoder fills the issue
 * slots the decimator's waves leave empty).  Same bytes, one call later.  sdrhip_rx_flush encodes and delivers the frames the
 * last call completed (end of stream, before switching the mode off, and before a sdrhip_rx_reconfigure that changes fecblk:
 * the waiting frames carry the old frame size; reconfigure refuses otherwise).  frames_out of a pipelined call must hold
 * sdrhip_rx_max_frames() frames per stream.
 * What it is for: the reference's delivery semantics, and an A / B partner.  It is NOT the fast path on an MI355X: both kernels run
 * at the board's power cap, co-resident they take the sum of their times (DESIGN.md "Whole pipes": 0.296-0.299 ms per step of the
 * headline bank against 0.260-0.276 in the default, immediate mode); a pipelined pipe also keeps the stream-order arrangement
 * (context option "rx_direct" applies to immediate pipes). */
int sdrhip_rx_set_pipelined(sdrhip_rx *rx, int on);
/* Input format of every later sdrhip_rx_process (host and device memory, immediate and pipelined) and sdrhip_rx_submit:
 * SDRHIP_IQ_S16 (the default), SDRHIP_IQ_U8 or SDRHIP_IQ_S8.  The RTL-SDR / HackRF sources widen their bytes on a host core
 * (RtlSdrSource.cpp:542-553, HackRFSource.cpp:661-674) and report get_sample_bits() = 8, which sdrdaemonrx hands to
 * Downsampler::process (sdrdaemonrx.cpp:619-643); here the bytes cross the host link as they are (2 bytes per sample instead of 4)
 * and a gfx950 kernel widens them into the decimator's int16 input on the device.  sample_bits stays the caller's choice in
 * sdrhip_rx_config (an RTL-SDR caller configures 8): the format does not imply a value.  8-bit device input: 16-byte aligned, the
 * stream stride a multiple of 8 samples (else SDRHIP_EALIGN); the caller's memory is only read.  Refused with SDRHIP_EINVAL,
 * nothing changed: an unknown format, asynchronous batches being filled or in flight, a pipelined pipe with undelivered frames
 * (sdrhip_rx_flush first). */
int sdrhip_rx_set_input_format(sdrhip_rx *rx, int fmt);
int sdrhip_rx_flush(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t *n_frames, int mem);
/* the decimator launch of the last sdrhip_rx_process call (see sdrhip_decimators_last_plan) */
int sdrhip_rx_last_plan(const sdrhip_rx *rx, sdrhip_decim_plan *out);
/* Zero-copy alternative for device-side consumers (what transmitUDP does when it sends straight
 * from m_txBlocks, UDPSinkFEC.cpp:259-282): call sdrhip_rx_process with frames_out = NULL and
 * mem = SDRHIP_MEM_DEVICE, then read the n_frames finished frames of stream s at
 * base + s * stream_stride_bytes (device memory, frame after frame).  The view stays valid until
 * the next sdrhip_rx_process / sdrhip_rx_destroy on this handle. */
int sdrhip_rx_frames_view(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes, size_t *n_frames);

/* Rx pipe, ragged: stream s takes n_in[s] device-rate samples whose first sample was taken at tv_sec[s] / tv_usec[s];
 * n_frames[s] = frames stream s completed; they land at frames_out + s * frame_stride_bytes as today.
 * n_in, tv_sec, tv_usec and n_frames are host arrays of nstreams entries.  Per stream the result is byte for byte what a one-stream
 * sdrhip_rx with the same config produces when it is fed stream s's samples with stream s's stamps, call after call: frames,
 * recovery blocks, meta blocks and frameIndex (each stream's m_frameCount wraps on its own).  A stream with n_in[s] below
 * 2^log2decim keeps its filter history, open frame and frame counter.  Input: as sdrhip_rx_process (host memory: only n_in[s]
 * samples of row s are read; device memory: its alignment rules, no sample past n_in[s] is read; sdrhip_rx_set_input_format
 * applies, or each stream's own format and the 4-byte stride unit of sdrhip_rx_set_stream_format).  frame_stride_bytes >= (largest n_frames) * (128 + nb_fec) * 512 when frames_out is given.  Once ragged calls leave the
 * streams at different frame positions: sdrhip_rx_process runs as a ragged call with equal counts and stamps (its *n_frames = the
 * largest per-stream count), sdrhip_rx_max_frames returns the maximum over the streams, sdrhip_rx_frames_view returns SDRHIP_EINVAL
 * while the delivered windows differ, sdrhip_rx_reconfigure moves each stream's open frame (the old-meta / new-fecblk rule applies per
 * stream), and sdrhip_rx_set_pipelined(on) / sdrhip_rx_submit return SDRHIP_EINVAL.  The decimator launch is chosen as for
 * sdrhip_decimate_ragged; on the matrix cores it stores straight into each stream's frame window (context option rx_direct, the
 * default; 0: stream order and a framing pass).  Refused with SDRHIP_EINVAL, nothing consumed (the next call continues
 * as if the refused one never happened): a NULL count, stamp or n_frames array, in_stride below the largest count, a frame stride
 * too small for the stream with the most frames, pipelined mode, asynchronous batches being filled or in flight. */
int sdrhip_rx_process_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride,
                             const uint32_t *tv_sec, const uint32_t *tv_usec, uint8_t *frames_out,
                             size_t frame_stride_bytes, size_t *n_frames, int mem);
/* zero-copy view after a ragged call: stream s's n_frames[s] frames start at base + s * stride + first_slot[s] * frame bytes
 * (first_slot and n_frames: host arrays of nstreams entries; valid until the next data call on the handle) */
int sdrhip_rx_frames_view_ragged(const sdrhip_rx *rx, const uint8_t **base, size_t *stream_stride_bytes,
                                 size_t *first_slot, size_t *n_frames);

/* Asynchronous host-pointer entry.  The reference's Rx chain is asynchronous end to end (source thread -> source_buffer ->
 * Downsampler::process -> output_buffer -> writer -> transmit thread, sdrdaemonrx.cpp:555-663): the frames of a block leave the
 * process long after it was pulled.  sdrhip_rx_submit takes one block of host samples per stream like sdrhip_rx_process
 * (SDRHIP_MEM_HOST) and returns at once: the block is appended to a pinned staging buffer -- or used IN PLACE when it lies in
 * sdrhip_host_alloc memory, which the caller then leaves untouched until the batch is collected -- and every `blocks` blocks go
 * out as one upload + launch + download on the context's stream.  sdrhip_rx_collect returns the finished frames of the OLDEST
 * batch ((128 + nb_fec) super blocks per frame, stream s at frames_out + s * frame_stride_bytes; frames_out has room for
 * max_frames frames per stream: a batch that holds more stays uncollected, *n_frames says how many, the call returns
 * SDRHIP_EINVAL; sdrhip_rx_max_frames() of the batch's samples bounds them -- in pipelined mode a batch delivers the frames the
 * PREVIOUS batch completed).  SDRHIP_OK always means: ONE batch was collected (*n_frames of it, possibly 0: blocks shorter than a
 * frame); SDRHIP_EBUSY: none was -- nothing submitted, or (wait = 0) the oldest batch is still in flight or being filled; wait = 1
 * blocks, outside the context lock (another thread may go on submitting), and launches a partly filled batch as it is (end of
 * stream).  At most `depth` batches are in flight; sdrhip_rx_submit
 * returns SDRHIP_EBUSY when the ring is full.  Defaults (no sdrhip_rx_set_async call): depth 4, one block per batch.  tv_sec /
 * tv_usec of a batch = those of its first block (frames are stamped by the sample clock from there, see sdrhip_rx_process).
 * Do not mix sdrhip_rx_process calls into a submit / collect sequence while batches are in flight. */
int sdrhip_rx_set_async(sdrhip_rx *rx, int depth, int blocks);
int sdrhip_rx_submit(sdrhip_rx *rx, const int16_t *iq_in, size_t n_in, size_t in_stride, uint32_t tv_sec, uint32_t tv_usec);
int sdrhip_rx_collect(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames, int wait);

/* Asynchronous ragged entry: the host-fed mode of a host with N sources, each delivering its own block size at its own rate.
 * sdrhip_rx_submit_ragged appends one block per stream to the batch being filled: stream s contributes n_in[s] samples (0 is
 * allowed, and so are counts below 2^log2decim).  The ring and the batch size are those of sdrhip_rx_set_async(depth, blocks);
 * it returns SDRHIP_EBUSY when every batch of the ring is in flight.  Rows: in_stride-strided (in_stride >= the largest count),
 * or SDRHIP_PACKED: back to back, row s starting at sample sum_{t<s} n_in[t].  sdrhip_rx_set_input_format applies; the counts
 * stay in samples (an 8-bit sample is 2 bytes).  (With sdrhip_rx_set_stream_format's array set: each stream's own format, packed
 * rows back to back in bytes, strided rows 4 * in_stride bytes apart.)  Packed input that lies wholly inside sdrhip_host_alloc memory is used IN PLACE
 * (the caller leaves it untouched until the batch is collected); anything else is copied into the pinned staging arena packed:
 * one memcpy per non-empty row, never the padding between a short row and the stride.
 * Per stream a batch is exactly one sdrhip_rx_process_ragged call: its count is the sum of the stream's counts over the batch's
 * blocks, its stamp is the stream's tv_sec[s] / tv_usec[s] of the batch's FIRST block.  Frames, recovery blocks, meta blocks,
 * frameIndex and the carried filter, frame and counter state are byte for byte what that sequence of synchronous ragged calls
 * produces (and so what one one-stream pipe per stream produces).  A batch moves what it carries: host to device the packed
 * sample bytes (sum of the counts x 4, or x 2 for 8-bit input), one copy per run of adjacent memory; device to host
 * sum_s n_frames[s] x (128 + nb_fec) x 512 bytes in one copy.  Both are counted in "h2d_bytes" / "d2h_bytes".  The per-batch
 * tables on top are NOT counted: at most 16 x (nstreams + 1) + 16 x (blocks x nstreams) + 16 + 4 x (frames of the batch) bytes
 * host to device (the packing table, the download's frame list).
 * sdrhip_rx_collect_ragged returns the OLDEST batch: stream s's n_frames[s] frames (host array of nstreams entries) at
 * frames_out + s * frame_stride_bytes, frame_stride_bytes >= (largest n_frames) x (128 + nb_fec) x 512 for more than one stream.
 * Its contract is sdrhip_rx_collect's: SDRHIP_OK = one batch collected (possibly with no frames); SDRHIP_EBUSY = none was
 * (nothing submitted, or with wait = 0 the oldest batch is still being filled or in flight); wait = 1 blocks outside the context
 * lock and launches a partly filled batch as it is; a stream with more than max_frames frames leaves the batch uncollected with
 * n_frames[] filled in and returns SDRHIP_EINVAL.
 * Refused with SDRHIP_EINVAL, nothing consumed (the next call continues as if the refused one never happened): a NULL count or
 * stamp array, an in_stride that is neither SDRHIP_PACKED nor >= the largest count, pipelined mode, a ragged submit / collect while
 * uniform batches are being filled or in flight, sdrhip_rx_submit / sdrhip_rx_collect / sdrhip_rx_process[_ragged] while ragged
 * batches are (a batch holds one kind; once they are collected the state carries over both ways).  A batch that fails before its
 * decimator launch is launched again by the next submit / collect; one that fails behind it is dropped, never replayed. */
#define SDRHIP_PACKED 0 /* in_stride value: rows back to back, row s starts at sample sum_{t<s} n_in[t] */
int sdrhip_rx_submit_ragged(sdrhip_rx *rx, const int16_t *iq_in, const size_t *n_in, size_t in_stride, const uint32_t *tv_sec,
                            const uint32_t *tv_usec);
int sdrhip_rx_collect_ragged(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames, size_t *n_frames, int wait);
/* Pinned host memory for the source side (the buffers a DeviceSource pushes): blocks submitted from it skip the staging copy. */
void *sdrhip_host_alloc(sdrhip_ctx *ctx, size_t bytes);
void sdrhip_host_free(sdrhip_ctx *ctx, void *p);

/* ------------------------------------------------------------ fused Tx pipe -- */
/* Bank of Tx chains: SDRdaemonFECBuffer decode (SDRdaemonFECBuffer.cpp:143-213) ->
 * getSlotData (:72-75) -> Upsampler::process (Upsampler.cpp:52-84), i.e. what
 * sdrdaemontx's main loop computes between recvfrom() and sink_buffer.push()
 * (sdrdaemontx.cpp:449-498).  rx = per stream nframes x 128 received super blocks (arrival
 * order); iq_out receives nframes * 16129 << log2interp samples per stream. */
typedef struct sdrhip_tx sdrhip_tx;
int sdrhip_tx_create(sdrhip_ctx *ctx, int nstreams, int log2interp, sdrhip_tx **out);
void sdrhip_tx_destroy(sdrhip_tx *tx);
/* Upsampler::configure's `interp` key (Upsampler.cpp:31-50) between two sdrhip_tx_process calls, the way
 * sdrdaemontx applies a control message (sdrdaemontx.cpp:381); the interpolator histories carry over. */
int sdrhip_tx_reconfigure(sdrhip_tx *tx, int log2interp);
int sdrhip_tx_process(sdrhip_tx *tx, const uint8_t *rx, const uint8_t *indices, size_t nframes,
                      size_t rx_stride_bytes, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
/* Pipelined mode (off by default).  The reference's Tx chain lives with one frame of latency already: SDRdaemonFECBuffer hands a
 * frame out when the NEXT frame's first block arrives (SDRdaemonFECBuffer.cpp:133-139), and a reader thread keeps receiving while
 * the main loop interpolates (sdrdaemontx.cpp:449-498).  With on != 0 a sdrhip_tx_process call decodes ITS batch on the
 * context's second stream (planner + syndrome decoder: VALU / LDS-latency work) while the first stream interpolates the batch
 * the PREVIOUS call decoded (store-bound), and DELIVERS that previous batch: iq_out / out_stride / *n_out describe the previous
 * batch's samples (sdrhip_tx_pending_samples() per stream before the call; 0 after the first call or a flush -- iq_out may then
 * be NULL).  Same samples, one call later; a waiting batch keeps the interpolation factor it was handed in with.
 * sdrhip_tx_flush delivers the batch the last call decoded (end of stream, before switching the mode off).  A DEVICE rx buffer
 * of a pipelined call is read by the second stream after the call returns: leave it untouched until the next
 * sdrhip_tx_process / sdrhip_tx_flush on this handle has returned.  (Context option "tx_overlap" = 0: the same one-call-late
 * delivery with both kernels on the first stream, the A / B partner.) */
int sdrhip_tx_set_pipelined(sdrhip_tx *tx, int on);
/* Output format of every later sdrhip_tx_process, sdrhip_tx_flush, sdrhip_tx_collect and sdrhip_tx_process_datagrams:
 * SDRHIP_IQ_S16 (the default) or SDRHIP_IQ_S8, the HackRF sink's bytes (HackRFSink.cpp:671-672: buf[2i] = real() >> 8,
 * buf[2i + 1] = imag() >> 8).  The interpolator's last stage narrows and stores 2 bytes per sample; host outputs download 2 bytes
 * per sample; block0_out is unchanged.  8-bit device output: 16-byte aligned, the stream stride a multiple of 8 samples (else
 * SDRHIP_EALIGN).  A batch takes the format in force when it is handed in (sdrhip_tx_process, sdrhip_tx_submit).  Refused with
 * SDRHIP_EINVAL, nothing changed: an unknown format, SDRHIP_IQ_U8 (no Tx radio takes it), asynchronous batches in flight, a
 * pipelined batch waiting (sdrhip_tx_flush first). */
int sdrhip_tx_set_output_format(sdrhip_tx *tx, int fmt);
int sdrhip_tx_flush(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t *n_out, int mem);
size_t sdrhip_tx_pending_samples(const sdrhip_tx *tx);
/* Asynchronous host-pointer entry, the Tx twin of sdrhip_rx_submit / sdrhip_rx_collect.  sdrdaemontx receives on a reader thread
 * while the main loop interpolates (sdrdaemontx.cpp:449-498) and its collector releases a frame one frame late
 * (SDRdaemonFECBuffer.cpp:133-139).  sdrhip_tx_submit takes ONE batch of received frames from host memory (rx, indices,
 * nframes, rx_stride_bytes as in sdrhip_tx_process; staged through pinned memory, or used in place when it lies in
 * sdrhip_host_alloc memory, which the caller then leaves untouched until the batch is collected), enqueues upload + decode +
 * interpolate + download on the context's stream and returns at once.  sdrhip_tx_collect returns the OLDEST batch: its
 * nframes * 16129 << log2interp samples per stream (stream s at iq_out + 2 * s * out_stride; iq_out has room for max_samples per
 * stream: a bigger batch stays uncollected, *n_out says how many, the call returns SDRHIP_EINVAL) and, when block0_out is not
 * NULL, the frames' meta blocks (super block 0: nstreams * nframes x 508 bytes, stream-major) -- with log2interp = 0 the two
 * together are exactly what SDRdaemonFECBuffer hands out per frame (getSlotData + the meta block, .cpp:72-110).  SDRHIP_OK: one
 * batch collected (*n_out samples per stream, *n_frames frames); SDRHIP_EBUSY: none -- nothing submitted, or (wait = 0) the oldest
 * batch is still in flight; wait = 1 blocks outside the context lock.  At most `depth` batches are in flight (default 4);
 * sdrhip_tx_submit returns SDRHIP_EBUSY when the ring is full.  The factor in force at submit time applies to the batch. */
int sdrhip_tx_set_async(sdrhip_tx *tx, int depth);
int sdrhip_tx_submit(sdrhip_tx *tx, const uint8_t *rx, const uint8_t *indices, size_t nframes, size_t rx_stride_bytes);
int sdrhip_tx_collect(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_samples, uint8_t *block0_out, size_t *n_out,
                      size_t *n_frames, int wait);

/* ------------------------------------------------------------ FEC buffer bank -- */
/* A bank of `nstreams` independent SDRdaemonFECBuffer instances (SDRdaemonFECBuffer.h, SDRdaemonFECBuffer.cpp:112-250) fed raw
 * datagrams: the collecting half of sdrdaemontx's receive path (frame change, first-128 policy, decode at the 128th block,
 * statistics) on the GPU, for many streams at once.  Each stream behaves exactly like one reference object fed the same datagrams
 * one at a time, whatever way its datagrams are cut into calls (a frame may begin in one call and end several calls later).
 * Differences: the initial slot (m_frameHead = -1) released by a stream's first datagram reads zero (the reference hands out
 * uninitialised memory); context option dec_strict applies as in sdrhip_fec_decode_frames (0, the default: every restored block
 * is delivered; 1: the reference's copy-back holes), dec_path and dec_plan apply, dec_max_rows does NOT: the bank passes the
 * decoder a bound it collected itself (the highest recovery row among the first 128 blocks of the batch's frames), so
 * "dec_rows_exceeded" never grows because of it.  A frame with a repeated original among its first 128 blocks is delivered as
 * received, the LAST copy of a repeated original in place (cm256_decode fails on such a frame; SDRHIP_FECBUF_DECODE_ERROR). */
typedef struct sdrhip_fecbuf sdrhip_fecbuf;
int sdrhip_fecbuf_create(sdrhip_ctx *ctx, int nstreams, sdrhip_fecbuf **out);
void sdrhip_fecbuf_destroy(sdrhip_fecbuf *b);
/* back to the constructor's state (m_frameHead = -1, min blocks 256, max recovery 0, zero meta) */
int sdrhip_fecbuf_reset(sdrhip_fecbuf *b);

#define SDRHIP_FECBUF_DECODED 1      /* m_decoded: the frame reached 128 blocks */
#define SDRHIP_FECBUF_META 2         /* m_metaRetrieved: block 0 was among its first 128 blocks */
#define SDRHIP_FECBUF_REPAIRED 4     /* decoded with recovery blocks: erased originals restored */
#define SDRHIP_FECBUF_DECODE_ERROR 8 /* decoded with recovery blocks, but an original arrived twice: left as received */
typedef struct {
    int32_t frame_index;    /* header.frameIndex of the released slot; -1 = the collector's initial slot */
    int32_t block_count;    /* m_blockCount: every datagram of the frame, not only the first 128 */
    int32_t recovery_count; /* m_recoveryCount: recovery blocks among the first 128 */
    uint32_t flags;         /* SDRHIP_FECBUF_* */
} sdrhip_fecbuf_frame;

/* SDRdaemonFECBuffer::writeAndRead over a batch: stream s gives n_dgrams[s] (host array) datagrams of 512 bytes, in arrival order,
 * at dgrams + s * dgram_stride_bytes.  Every frame those datagrams release is written, in release order, to
 * data_out + s * data_stride_bytes (127 x 508 bytes each = getSlotData, frame after frame), its block 0 (508 bytes: the meta
 * block) to block0_out + (s * max_frames + k) * 508 (block0_out may be NULL), and its record to info_out[s * max_frames + k]
 * (host).  n_frames[s] (host) receives the count of stream s.  A stream that releases more than max_frames frames: the call
 * returns SDRHIP_EINVAL with every stream's count in n_frames and consumes NOTHING (call again with room).  dgrams / data_out /
 * block0_out are in `mem` memory: SDRHIP_MEM_HOST (staged through pinned memory; used in place when the datagrams lie in
 * sdrhip_host_alloc memory; returns with the outputs written) or SDRHIP_MEM_DEVICE (dgrams and dgram_stride_bytes 16-byte
 * aligned, data_out / block0_out and data_stride_bytes 4-byte aligned; the outputs are enqueued on the context's stream and not
 * synchronised).  Either way the call synchronises once, to read back the frame counts. */
int sdrhip_fecbuf_write_and_read(sdrhip_fecbuf *b, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                 uint8_t *data_out, size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames,
                                 sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem);
/* The getters of SDRdaemonFECBuffer.h:107-126 for one stream (any pointer may be NULL): getCurNbBlocks, getCurNbRecovery,
 * getMinNbBlocks, getMaxNbRecovery (the last two reset when read, like the reference's), getCurrentMeta, getOutputMeta (20-byte
 * MetaDataFEC, zero-padded to 24).  Synchronises the context's stream. */
int sdrhip_fecbuf_stats(sdrhip_fecbuf *b, int stream, int *cur_nb_blocks, int *cur_nb_recovery, int *min_nb_blocks,
                        int *max_nb_recovery, uint8_t current_meta[24], uint8_t output_meta[24]);

/* ------------------------------------------------------------ Tx pipe fed datagrams -- */
/* sdrdaemontx's receive chain for every stream of the bank (UDPSourceFEC::read -> SDRdaemonFECBuffer::writeAndRead ->
 * Upsampler::process): datagrams in, interpolated samples out.  dgrams, n_dgrams, dgram_stride_bytes, max_frames, block0_out,
 * info_out, n_frames and mem mean what they mean for sdrhip_fecbuf_write_and_read; the handle's collector (one
 * SDRdaemonFECBuffer per stream, created on the first call) behaves exactly like the bank.  Stream s gets
 * n_frames[s] * 16129 << log2interp samples at iq_out + 2 * s * out_stride (room for max_frames * 16129 << log2interp per stream;
 * samples past a stream's count are unspecified).  Each stream keeps one set of interpolator histories, shared with
 * sdrhip_tx_process (a stream of the handle is one Upsampler); a stream that releases no frame keeps them as they are, and
 * sdrhip_tx_reconfigure applies to the next call of either entry.  SDRHIP_EINVAL with nothing consumed (neither the collector
 * nor any history moves; n_frames holds every stream's count) when a stream would release more than max_frames, and while the
 * handle is pipelined or asynchronous batches are in flight.  Device memory: iq_out 16-byte aligned and out_stride a multiple
 * of 4 samples (as sdrhip_tx_process), block0_out 4-byte aligned; the call synchronises once, for the bank's read-back of the
 * frame counts.  Host memory: the call returns with the outputs written. */
int sdrhip_tx_process_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                int16_t *iq_out, size_t out_stride, size_t max_frames, uint8_t *block0_out,
                                sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem);
/* the handle's collector (borrowed; destroyed with the handle) for sdrhip_fecbuf_stats / sdrhip_fecbuf_reset */
int sdrhip_tx_collector(sdrhip_tx *tx, sdrhip_fecbuf **out);
/* Asynchronous datagram batches, the datagram twin of sdrhip_tx_submit / sdrhip_tx_collect: sdrdaemontx's reader thread receives
 * while its main loop interpolates (sdrdaemontx.cpp:449-498).  sdrhip_tx_submit_datagrams takes ONE batch from host memory:
 * stream s gives n_dgrams[s] datagrams of 512 bytes (counts may differ and may be 0) at dgrams + s * dgram_stride_bytes, or, with
 * dgram_stride_bytes = SDRHIP_PACKED, back to back (stream s at dgrams + 512 * sum_{t<s} n_dgrams[t]).  The datagrams are staged
 * into pinned memory (the buffer is the caller's again on return) or, when they lie in sdrhip_host_alloc memory, uploaded in
 * place (leave them untouched until the batch is collected).  The call enqueues upload, collection, decode, interpolation at the
 * factor in force and download in the output format in force, and returns with NO synchronisation (the first batch after the
 * handle's collector was created, reset or fed by sdrhip_tx_process_datagrams reads its state back once).  The batch keeps that
 * factor and format.  sdrhip_tx_collect_datagrams returns the OLDEST batch, meaning what sdrhip_tx_process_datagrams means for
 * the same datagrams: stream s gets n_frames[s] * 16129 << log2interp samples at iq_out + 2 * s * out_stride (8-bit output:
 * byte addressing as for sdrhip_tx_collect), the released frames' meta blocks at block0_out + (s * max_frames + k) * 508
 * (block0_out may be NULL) and records at info_out[s * max_frames + k].  A stream that released more than max_frames, or an
 * out_stride below the batch's largest stream: SDRHIP_EINVAL with every stream's count in n_frames, the batch stays (call again
 * with room).  SDRHIP_EBUSY: nothing submitted, or (wait = 0) the oldest batch is still in flight; wait = 1 blocks outside the
 * context lock.  The ring depth is sdrhip_tx_set_async's (default 4); a full ring makes the submit return SDRHIP_EBUSY.  The
 * collector and the histories are the handle's (sdrhip_tx_collector, sdrhip_tx_process_datagrams, sdrhip_tx_process):
 * synchronous calls before and after a run of batches continue the same streams, and sdrhip_fecbuf_stats reports the state after
 * every batch submitted so far.  While datagram batches are in flight, SDRHIP_EINVAL with nothing consumed from
 * sdrhip_tx_submit / _collect, sdrhip_tx_process, sdrhip_tx_process_datagrams, sdrhip_tx_set_output_format, sdrhip_tx_set_async,
 * sdrhip_tx_set_pipelined(1), and sdrhip_fecbuf_reset / sdrhip_fecbuf_write_and_read on the handle's collector; the datagram
 * entries refuse the same way while batches of received frames are in flight, in pipelined mode and while a pipelined batch
 * waits.  sdrhip_tx_reconfigure applies to later submits.  A submit that fails before the collector's scatter launch consumes
 * nothing; one that fails behind it loses the batch (never replayed). */
int sdrhip_tx_submit_datagrams(sdrhip_tx *tx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes);
int sdrhip_tx_collect_datagrams(sdrhip_tx *tx, int16_t *iq_out, size_t out_stride, size_t max_frames, uint8_t *block0_out,
                                sdrhip_fecbuf_frame *info_out, size_t *n_frames, int wait);

/* ------------------------------------------------------------ Rx pipe fed datagrams -- */
/* A hub between a fast link and a slow one: per stream, sdrdaemontx's receive half (UDPSourceFEC::read ->
 * SDRdaemonFECBuffer::writeAndRead, sdrdaemontx.cpp:449-498) chained to sdrdaemonrx's send half (Downsampler::process ->
 * UDPSinkFEC::write, sdrdaemonrx.cpp:619-644).  Radio heads that cannot afford the half-band cascades send undecimated IQSample
 * streams as FEC-protected datagrams; this call repairs the losses, decimates, re-frames and re-protects them.
 * Collect: dgrams, n_dgrams, dgram_stride_bytes, info_out and mem mean what they mean for sdrhip_fecbuf_write_and_read;
 * info_out[s * max_released + k] is the record of the k-th frame stream s released, n_released[s] (host) their count.  The
 * handle's collector (one SDRdaemonFECBuffer per stream, created on the first call) behaves exactly like the bank (dec_strict,
 * dec_path, dec_plan apply; the initial slot's zero payload is a released frame like any other: sdrdaemontx hands it to its
 * Upsampler too).
 * Join: the released payloads of stream s (16129 samples each), in release order, go behind the samples the stream holds back
 * from earlier calls (its carry).  Of carry + 16129 * n_released[s] samples the largest multiple of U is decimated, the rest --
 * 63 samples at the most -- is the new carry.  U = 2^log2decim, but 4 for log2decim = 1 with fcpos inf / sup (decimate2_inf /
 * _sup walk the input in fours, Decimators.cpp:48,76).  The carry is the remainder buffer a host loop would keep between
 * Downsampler::process calls, not decimator state: it survives sdrhip_rx_reconfigure (a new U applies to the next call),
 * sdrhip_rx_process[_ragged] neither read nor clear it, sdrhip_fecbuf_reset on the handle's collector clears it together with
 * the collector.
 * Decimate, frame, encode: one sdrhip_rx_process_ragged step with those counts; tv_sec[s] / tv_usec[s] (host arrays) stamp the
 * first sample fed.  Its rules apply unchanged: a stream fed nothing keeps its filter history, open frame and counter; frames
 * land at frames_out + s * frame_stride_bytes, n_frames[s] (host) of them; frames_out = NULL with SDRHIP_MEM_DEVICE leaves them
 * to sdrhip_rx_frames_view_ragged; sdrhip_rx_last_plan reports the launch; streams stand at different frame positions
 * afterwards.  sdrhip_rx_set_input_format does not apply (the wire carries IQSample).  Size frames_out with
 * sdrhip_rx_max_frames(rx, 16129 * max_released + 63).
 * SDRHIP_EINVAL with nothing consumed (collector, carry, histories, open frames and counters stay as they were): a stream that
 * would release more than max_released (n_released holds every stream's count), NULL count or stamp arrays, a frame stride too
 * small for the stream with the most frames, pipelined mode, asynchronous batches being filled or in flight.
 * Device memory: dgrams as sdrhip_fecbuf_write_and_read, frames_out as sdrhip_rx_process_ragged; the call synchronises once, for
 * the collector's read-back of the release counts.  Host memory: the call returns with the frames written; only datagrams,
 * frames, records and counts cross the link, the samples between collector and decimator stay on the device. */
int sdrhip_rx_process_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                                const uint32_t *tv_sec, const uint32_t *tv_usec, size_t max_released,
                                uint8_t *frames_out, size_t frame_stride_bytes, sdrhip_fecbuf_frame *info_out,
                                size_t *n_released, size_t *n_frames, int mem);
/* the handle's collector (borrowed; destroyed with the handle) for sdrhip_fecbuf_stats / sdrhip_fecbuf_reset */
int sdrhip_rx_collector(sdrhip_rx *rx, sdrhip_fecbuf **out);
/* carry: host array of nstreams entries, the samples each stream holds back (0 .. 63) */
int sdrhip_rx_carry(const sdrhip_rx *rx, size_t *carry);
/* Asynchronous datagram batches, the datagram twin of sdrhip_rx_submit_ragged / sdrhip_rx_collect_ragged and the Rx twin of
 * sdrhip_tx_submit_datagrams: a hub's reader thread keeps receiving while its main loop works (sdrdaemontx.cpp:449-498), and
 * UDPSinkFEC::write returns at once (UDPSinkFEC.cpp:193-211).  sdrhip_rx_submit_datagrams takes ONE batch from host memory:
 * stream s gives n_dgrams[s] datagrams of 512 bytes (counts may differ and may be 0) at dgrams + s * dgram_stride_bytes, or, with
 * dgram_stride_bytes = SDRHIP_PACKED, back to back (stream s at dgrams + 512 * sum_{t<s} n_dgrams[t]); tv_sec[s] / tv_usec[s]
 * (host arrays) stamp the first sample stream s feeds its decimator in this batch.  The datagrams are staged into pinned memory
 * (the buffer is the caller's again on return) or, when they lie in sdrhip_host_alloc memory, uploaded in place (leave them
 * untouched until the batch is collected).  The call enqueues upload, collection, decode, the join behind the carry, the ragged
 * decimate / frame / encode step at the configuration in force, the delivery and ONE download, and returns with NO
 * synchronisation: every count comes from the host's shadow of the classification (the first batch after the handle's collector
 * was created, reset or fed by sdrhip_rx_process_datagrams reads its state back once; rows or frame areas that grow synchronise
 * once; every pinned table of a batch belongs to its ring slot, so a submit waits for no earlier batch).  A batch means exactly one sdrhip_rx_process_datagrams call with the same datagrams and stamps: frames, recovery blocks,
 * meta blocks, frameIndex, records, and the collector state, carry, filter histories, open frames and counters left behind are
 * byte for byte those of that sequence of synchronous calls; synchronous calls before and after a run of batches continue the same
 * streams, and sdrhip_rx_carry / sdrhip_fecbuf_stats report the state after every batch submitted so far.
 * sdrhip_rx_collect_datagrams returns the OLDEST batch: stream s's n_frames[s] frames of (128 + nb_fec) x 512 bytes at
 * frames_out + s * frame_stride_bytes and its n_released[s] records at info_out[s * max_released + k] (both counts: host arrays
 * of nstreams entries).  SDRHIP_OK: one batch collected, possibly with no frames.  SDRHIP_EBUSY: none was -- nothing submitted,
 * or (wait = 0) the oldest batch is still in flight; wait = 1 blocks outside the context lock.  A stream with more than max_frames
 * frames or more than max_released records, or a frame stride below the stream with the most frames: SDRHIP_EINVAL with both
 * count arrays filled in, the batch stays (call again with room).  The ring depth is sdrhip_rx_set_async's (default 4; its
 * `blocks` does not apply: one submit is one batch); a full ring makes the submit return SDRHIP_EBUSY with nothing consumed.
 * One kind of batch at a time: the datagram submit is refused (SDRHIP_EINVAL, nothing consumed) in pipelined mode, while uniform
 * or ragged batches are being filled or in flight, for NULL count or stamp arrays and for a stride that is neither SDRHIP_PACKED
 * nor at least the largest count x 512.  While datagram batches are in flight, SDRHIP_EINVAL with nothing consumed from
 * sdrhip_rx_submit[_ragged], sdrhip_rx_collect[_ragged], sdrhip_rx_process[_ragged], sdrhip_rx_process_datagrams,
 * sdrhip_rx_set_input_format, sdrhip_rx_set_async, sdrhip_rx_set_pipelined(1), and sdrhip_fecbuf_reset /
 * sdrhip_fecbuf_write_and_read on the handle's collector.  sdrhip_rx_reconfigure is allowed at any time and applies to later
 * submits: batches in flight keep the configuration (and frame size) they were submitted with; a fecblk change waits for them to
 * finish on the device (they are still collected as usual).  A submit that fails before the collector's scatter launch consumes
 * nothing, and everything the batch needs is allocated before that launch (but the decimator's stream-order rows, should a
 * matrix-core launch the sizes counted on not apply); one that fails behind it loses the batch (never replayed).  Link traffic ("h2d_bytes" / "d2h_bytes"): up exactly
 * sum n_dgrams x 512, down exactly sum n_frames x (128 + nb_fec) x 512 + sum n_released x 16 in one copy. */
int sdrhip_rx_submit_datagrams(sdrhip_rx *rx, const uint8_t *dgrams, const size_t *n_dgrams, size_t dgram_stride_bytes,
                               const uint32_t *tv_sec, const uint32_t *tv_usec);
int sdrhip_rx_collect_datagrams(sdrhip_rx *rx, uint8_t *frames_out, size_t frame_stride_bytes, size_t max_frames,
                                size_t max_released, sdrhip_fecbuf_frame *info_out, size_t *n_released, size_t *n_frames, int wait);

/* ------------------------------------------------------------ Tagged datagram batches -- */
/* A hub receives on ONE socket (recvmmsg): one array of 512-byte datagrams from all its radio heads, interleaved in arrival order.
 * The datagram header (frameIndex, blockIndex, filler) does not name the stream; the source address does, and only the host sees
 * it.  The tagged entries take that array as it is: dgrams holds n_total datagrams of 512 bytes back to back, in arrival order;
 * stream_of[i] (host array) is the stream of datagram i, or SDRHIP_DGRAM_SKIP for one that belongs to no stream of the bank
 * (unknown peer, wrong length).
 * Meaning: a tagged call is the untagged call of the same name with SDRHIP_PACKED input in which stream s's row is the subsequence
 * of the datagrams tagged s, in arrival order; skipped datagrams are in no row.  Everything else -- outputs, records, counts,
 * collector state, carry, histories, open frames, counters, the host's shadow, the refusals with nothing consumed -- is byte for
 * byte what the untagged call gives for those rows and leaves behind.  A batch submitted tagged is collected with
 * sdrhip_tx_collect_datagrams / sdrhip_rx_collect_datagrams; tagged and untagged calls may alternate on one handle.
 * How: the host walks the tags and the 4-byte headers once, in arrival order (the headers feed its shadow of the classification,
 * as they do for an untagged batch), and gives every datagram its place among its stream's; the array goes up unsorted with that
 * table, and one kernel (KX) puts it in the order the collector's passes read.  No host core touches a payload.
 * SDRHIP_EINVAL with nothing consumed, on top of everything the untagged twin refuses: a tag that is >= nstreams and not
 * SDRHIP_DGRAM_SKIP, stream_of == NULL with n_total > 0, a bank of more than 65535 streams.  The tags are checked before anything
 * is staged or moved.
 * Memory: for the two submits dgrams is host memory, used in place when it lies in sdrhip_host_alloc memory (recvmmsg straight
 * into it; leave it untouched until the batch is collected) and staged with ONE memcpy otherwise (the buffer is the caller's again
 * on return).  For the bank call mem means what it means for sdrhip_fecbuf_write_and_read; stream_of is always host memory; with
 * SDRHIP_MEM_DEVICE dgrams must be 16-byte aligned.
 * Link traffic of a submit ("h2d_bytes"): 512 bytes per datagram, skipped ones included, and 4 bytes per datagram for the table
 * of places; nothing per stream.  Down ("d2h_bytes"): what the untagged twin brings down. */
#define SDRHIP_DGRAM_SKIP 0xffffu   /* a datagram that belongs to no stream of the bank (unknown peer, wrong length) */
int sdrhip_fecbuf_write_and_read_tagged(sdrhip_fecbuf *b, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total,
                                        uint8_t *data_out, size_t data_stride_bytes, uint8_t *block0_out, size_t max_frames,
                                        sdrhip_fecbuf_frame *info_out, size_t *n_frames, int mem);
int sdrhip_tx_submit_datagrams_tagged(sdrhip_tx *tx, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total);
int sdrhip_rx_submit_datagrams_tagged(sdrhip_rx *rx, const uint8_t *dgrams, const uint16_t *stream_of, size_t n_total,
                                      const uint32_t *tv_sec, const uint32_t *tv_usec);

/* ------------------------------------------------------------ Rx egress: one departure-order array -- */
/* The mirror of the tagged submit.  sdrhip_rx_collect_ragged / sdrhip_rx_collect_datagrams hand a batch back per stream, stream
 * after stream, one memcpy per stream; a hub that sends what it was handed puts stream 0's n_frames x (128 + nb_fec) datagrams on
 * the wire back to back, then stream 1's.  The reference never does that to a receiver: UDPSinkFEC::transmitUDP sleeps txDelay
 * between any two datagrams of a stream (UDPSinkFEC.cpp:259-282; the control channel's txdelay key, sdrdaemonrx.cpp:607-613),
 * because receivers with small socket buffers drop bursts.  A bank of N streams gives every receiver that gap for free: datagram
 * j of every stream before datagram j + 1 of any.
 * sdrhip_rx_set_egress sets a host-side mode (nothing is enqueued, nothing waited for) for the batches launched LATER by
 * sdrhip_rx_submit_ragged, sdrhip_rx_submit_datagrams and sdrhip_rx_submit_datagrams_tagged; a batch keeps the order it was
 * launched with.  SDRHIP_EINVAL, nothing changed: an unknown order, a NULL handle, a batch being filled, a bank of more than 65535
 * streams.  While the order is not SDRHIP_EGRESS_OFF, sdrhip_rx_submit (uniform batches) returns SDRHIP_EINVAL with nothing
 * consumed: a ragged submit with equal counts does that job.  With SDRHIP_EGRESS_OFF, the default, every entry launches and
 * returns exactly what it did before this mode existed.
 * Departure order (SDRHIP_EGRESS_ROUND_ROBIN).  B = blocks_per_frame = 128 + the nb_fec the batch was submitted with; stream s
 * delivered F_s = n_frames[s] frames, that is D_s = F_s B datagrams in the reference's wire order (frame after frame, blocks
 * 0 .. B - 1 inside a frame, UDPSinkFEC.cpp:259).  The array is rounds j = 0, 1, 2, ... concatenated; round j holds datagram j of
 * every stream with D_s > j, streams in ascending order; stream_of[i] names the stream of entry i.  Per stream, the subsequence is
 * byte for byte what the stream-order collect returns for that stream; collector state, carry, histories, open frames, counters
 * and records are those of the same batch in stream order.
 * sdrhip_rx_collect_egress returns the OLDEST batch, of either kind, that was launched with an order.  n_frames: host array of
 * nstreams entries, required.  A datagram batch: n_released is required and the records land at info_out[s * max_released + k];
 * a stream with more than max_released records: SDRHIP_EINVAL with both count arrays filled, the batch stays.  A ragged batch:
 * info_out and n_released may be NULL; n_released, when given, is zero-filled.  SDRHIP_OK: one batch collected (one that
 * completed no frame: n_dgrams = 0).  SDRHIP_EBUSY: none was -- nothing submitted, or (wait = 0) the oldest batch is still in
 * flight; wait = 1 launches a ragged batch that is still being filled and blocks outside the context lock.  One kind of collect
 * per batch: sdrhip_rx_collect_ragged / sdrhip_rx_collect_datagrams on a batch launched with an order, and
 * sdrhip_rx_collect_egress on a stream-order batch, return SDRHIP_EINVAL and the batch stays.
 * Lending: out->dgrams and out->stream_of point into the batch's own ring slot -- its pinned download buffer and its tag array.
 * No host core copies a payload byte.  They stay valid and unchanged until sdrhip_rx_release_egress, the next successful
 * sdrhip_rx_collect_egress (which releases implicitly) or sdrhip_rx_destroy.  A lent batch occupies its ring slot: a submit that
 * finds every slot in flight or lent returns SDRHIP_EBUSY with nothing consumed (at depth 1: release before the next submit), and
 * sdrhip_rx_set_async and sdrhip_rx_set_input_format are refused while a batch is lent.  A lent batch is not in flight: once every
 * batch has been collected, lent or not, the synchronous entries and sdrhip_fecbuf_* on the collector work as after the last
 * stream-order collect.  sdrhip_rx_release_egress with nothing lent returns SDRHIP_OK.
 * How: one kernel (KR) in the place of the stream-order delivery writes the batch's one download buffer in departure order, from
 * a table of one entry per delivered frame that the host derives from its own counts; the host writes the tags from the same
 * counts, they never cross the link.  Everything the order needs is allocated before the batch consumes anything.  Link traffic
 * is the stream-order batch's: down ("d2h_bytes") exactly sum n_frames x B x 512 + sum n_released x 16 in one copy.
 * Paced order (SDRHIP_EGRESS_PACED).  Round robin keeps "no receiver sees a burst" only while every stream of a batch delivers
 * the same number of datagrams: a stream with more than the others sends its whole surplus back to back at the array's end (four
 * streams with 4, 1, 1, 1 frames of 136: 408 consecutive datagrams of stream 0).  The reference never bursts: every sdrdaemonrx
 * process spaces its OWN datagrams evenly, so N processes side by side put a rate-proportional interleave on the wire.  The paced
 * order is that interleave.  Stream s delivers D_s datagrams in wire order (D_s = F_s B, or F_s B_s with B_s = 128 + nb_fec[s]
 * under sdrhip_rx_set_stream_fec with differing counts); datagram j of stream s has the departure key
 *     k(s, j) = (2 j + 1) / (2 D_s),
 * the midpoint of its share of the batch period, and the array lists all datagrams by ascending key, ties by ascending stream.
 * Keys are compared exactly (64-bit cross products, no floating point); a batch with a D_s of 2^31 or more is refused with
 * SDRHIP_EDEVICE like any batch the index types cannot hold, never truncated.  Guarantee: between two consecutive datagrams of
 * stream s lie floor(D_t / D_s) or ceil(D_t / D_s) datagrams of every other stream t, never more and never fewer.  Equal counts
 * give exactly the round-robin array, byte for byte.  A sender that wants the reference's timing sends entry i of n at
 * (i + 1/2) / n of the batch period.  Everything above holds for it unchanged: it serves sdrhip_rx_submit_ragged,
 * sdrhip_rx_submit_datagrams and sdrhip_rx_submit_datagrams_tagged, is collected by sdrhip_rx_collect_egress (blocks_per_frame and
 * sdrhip_rx_egress_stream_blocks as for round robin), lends the same buffers, and batches of both orders may sit in the ring
 * together, each collected in the order it was launched with.  How: the destinations of a stream are no constant-stride runs, so
 * one kernel (KP) gathers by destination through a table of 4 bytes per datagram (16 bytes per stream in front) that the host
 * makes, with the tags, in one merge over the streams; the table's upload is not counted in "h2d_bytes", like KR's
 * table, and "d2h_bytes" is the round-robin batch's.
 * Not covered: uniform batches, the synchronous entries, a device-resident view of the array, the send itself, the Tx pipe. */
#define SDRHIP_EGRESS_OFF 0          /* default: frames per stream, sdrhip_rx_collect_ragged / _datagrams */
#define SDRHIP_EGRESS_ROUND_ROBIN 1  /* one departure-order array per batch, sdrhip_rx_collect_egress */
#define SDRHIP_EGRESS_PACED 2        /* ... in ascending departure key: streams with unequal counts never burst */
typedef struct {
    const uint8_t *dgrams;      /* n_dgrams x 512 bytes in departure order (lent) */
    const uint16_t *stream_of;  /* n_dgrams tags: the stream of datagram i (lent) */
    size_t n_dgrams;            /* = blocks_per_frame x sum n_frames[s] */
    size_t blocks_per_frame;    /* 128 + the nb_fec the batch was submitted with */
} sdrhip_rx_egress;
int sdrhip_rx_set_egress(sdrhip_rx *rx, int order);
int sdrhip_rx_collect_egress(sdrhip_rx *rx, sdrhip_rx_egress *out, size_t *n_frames, size_t max_released,
                             sdrhip_fecbuf_frame *info_out, size_t *n_released, int wait);
int sdrhip_rx_release_egress(sdrhip_rx *rx);

/* ---- Per-stream fecblk: the recovery block count of every stream of a bank, from the meta block to the egress array.
 * In the reference fecblk is set per process, that is per stream: the control channel's fecblk key calls
 * UDPSink::setNbBlocksFEC on that process's own sink (sdrdaemonrx.cpp:599-605); the count enters the meta block's nbFECBlocks
 * byte and the CRC over it (UDPSinkFEC.cpp:160-165) and sizes the frame's encoding (UDPSinkFEC.cpp:228-256).  A hub whose
 * clients sit behind links of different quality -- fecblk 4 on the LAN, 32 behind a lossy bridge -- keeps them in ONE bank.
 * sdrhip_rx_set_stream_fec: nb_fec = host array of nstreams entries, each 0..128; NULL = bank-wide again (cfg.nb_fec).
 * Contract.  Per stream the result is byte for byte that of a one-stream sdrhip_rx whose config carries nb_fec[s]: the meta
 * block's nbFECBlocks byte, the CRC over it, the recovery blocks computed over that block 0, the recovery headers.  A later call
 * acts on stream s exactly like sdrhip_rx_reconfigure with the new value on that one-stream pipe at the same point: the frame
 * being filled keeps the meta block it was opened with and is encoded with the count in force when it completes.
 * The config: while the array is set cfg.nb_fec is unused; sdrhip_rx_reconfigure does not clear the array, and neither does
 * sdrhip_rx_reset_streams (it is configuration, like the stream meta arrays); export and import of a stream are untouched.
 * Layout: the frame area keeps ONE slot pitch, slot_blocks = 128 + max_s nb_fec[s] (a call that changes it moves the open
 * frames the way a fecblk change of sdrhip_rx_reconfigure does); a frame of stream s holds 128 + nb_fec[s] valid super blocks,
 * the rest of its slot is unspecified.  sdrhip_rx_frames_view_ragged shows slots at that pitch; sdrhip_rx_get_stream_fec
 * reports a stream's count and the pitch.
 * Entries: while the array is set every step is the ragged step: sdrhip_rx_process, sdrhip_rx_submit and
 * sdrhip_rx_set_pipelined(1) return SDRHIP_EINVAL with nothing consumed.  The setter itself is refused, nothing changed, in
 * pipelined mode, while batches are being filled or in flight, while a batch is lent, and for a count outside 0..128.  A handle
 * on which the setter was never called launches exactly what it launched before.  An array of equal entries is allowed and
 * behaves, layout and delivery, like that bank-wide count.
 * Synchronous delivery (sdrhip_rx_process_ragged, sdrhip_rx_process_datagrams) with differing counts: stream s's frames land at
 * frames_out + s * frame_stride_bytes as 128 + nb_fec[s] super blocks each, frame after frame -- dense per stream, the
 * one-stream pipe's bytes; frame_stride_bytes must hold the largest n_frames[s] * (128 + nb_fec[s]) * 512.
 * Asynchronous delivery: a batch submitted while the array holds differing values is delivered in departure order only; with
 * SDRHIP_EGRESS_OFF sdrhip_rx_submit_ragged, sdrhip_rx_submit_datagrams and sdrhip_rx_submit_datagrams_tagged return
 * SDRHIP_EINVAL with nothing consumed (sdrhip_rx_set_egress first).  A batch keeps the counts it was submitted with.
 * Egress: the order's definition stands -- round j holds datagram j of every stream with D_s > j, streams ascending -- with
 * D_s = n_frames[s] * (128 + nb_fec[s]).  For such a batch sdrhip_rx_egress.blocks_per_frame is 0 and
 * sdrhip_rx_egress_stream_blocks fills `blocks` (nstreams entries) with each stream's 128 + nb_fec[s], valid while the batch is
 * lent (SDRHIP_EINVAL when none is; for a batch of equal frames every entry is blocks_per_frame).  The download holds exactly
 * sum n_frames[s] * (128 + nb_fec[s]) * 512 + sum n_released[s] * 16 bytes.
 * How: the ragged rows carry each stream's third meta word; recovery row r of CM256 does not depend on the count, so the frames
 * are encoded in at most three launches (one per encoder form) with the largest count of each group; a stream's end can fall
 * inside another stream's frame, so the delivery kernel (KR) moves runs of constant stride, at most sum n_frames + S (S - 1).
 * Not covered: the stream-order gather and KD for differing counts (departure order only), the uniform step, pipelined mode,
 * per-stream decimation, Fc position or sample size, the Tx pipe. */
int sdrhip_rx_set_stream_fec(sdrhip_rx *rx, const int *nb_fec);
int sdrhip_rx_get_stream_fec(const sdrhip_rx *rx, int stream, int *nb_fec, int *slot_blocks);
int sdrhip_rx_egress_stream_blocks(const sdrhip_rx *rx, size_t *blocks);

/* ---- Per-stream sample bits: 8-, 12- and 16-bit radios in one bank.
 * In the reference the sample size is per process, that is per stream: srcsdr->get_sample_bits() goes into Downsampler::process /
 * rescale (sdrdaemonrx.cpp:619-620, 639-640) and, as the decimator returns it, into UDPSink::setSampleBits / setSampleBytes
 * (sdrdaemonrx.cpp:622-623, 642-643).  RTL-SDR and HackRF heads say 8 (RtlSdrSource.cpp:549, HackRFSource.cpp:669), Airspy and
 * BladeRF 12, the test source 16.  The size changes the last operation of a cascade alone -- `x << norm_shift >> trunk_shift` in
 * front of the int16 truncation (Decimators.cpp:27-32, 43-44, 52-53, 62 and every decimateN) -- and two bytes of the meta block.
 * sdrhip_rx_set_stream_bits: sample_bits = host array of nstreams entries, each 1..16; NULL = bank-wide again (cfg.sample_bits).
 * sdrhip_rx_get_stream_bits: either pointer may be NULL; *sample_bits = the stream's size, *frame_bits = what the next frame the
 * stream opens says in its sampleBits byte.
 * Contract.  Per stream the result is byte for byte that of a one-stream sdrhip_rx whose config carries sample_bits[s]: the sample
 * values, bytes 8 (sampleBytes = (bits' - 1) / 8 + 1) and 9 (sampleBits = bits') of the meta block with bits' the size the
 * decimator returns for (log2decim, sample_bits[s]), the CRC over them, the recovery blocks computed over that block 0.  A later
 * call acts on stream s exactly like sdrhip_rx_reconfigure with the new sample_bits on that one-stream pipe at the same point: the
 * frame being filled keeps the meta block it was opened with (UDPSinkFEC.cpp:160-165), samples decimated from then on take the
 * new shift.
 * The config: while the array is set cfg.sample_bits is unused; sdrhip_rx_reconfigure does not clear the array, and neither does
 * sdrhip_rx_reset_streams; export and import of a stream are untouched (the bits are configuration: the destination's apply).  A
 * log2decim change through sdrhip_rx_reconfigure changes every stream's frame_bits by the same rule.
 * Entries: while the array is set every step is the ragged step: sdrhip_rx_process, sdrhip_rx_submit and
 * sdrhip_rx_set_pipelined(1) return SDRHIP_EINVAL with nothing consumed.  An array of equal entries is allowed and delivers the
 * bytes of that bank-wide value.  It holds through sdrhip_rx_process_ragged, sdrhip_rx_submit_ragged / _collect_ragged,
 * sdrhip_rx_process_datagrams, sdrhip_rx_submit_datagrams[_tagged] / _collect_datagrams and sdrhip_rx_collect_egress, and
 * together with the stream meta arrays, follow meta (whose rule 5 then speaks of the stream's own size) and the fecblk array in
 * any combination; the rules for differing fecblk (departure order only) stand as they are.
 * The setter changes host arrays alone: nothing is enqueued, nothing waited for.  It is allowed at any time, also with batches in
 * flight; a batch takes the values when it takes its sdrhip_rx_config (the rule of sdrhip_rx_set_stream_meta).  It is refused,
 * nothing changed, for a NULL handle, a value outside 1..16, a pipelined pipe or one with late frames waiting.  A handle on which
 * the setter was never called launches the same kernels in the same order with the same results.
 * How: every ragged launch takes the shift pair from its stream's row of the per-call table (one word) instead of the launch
 * arguments -- the filter-less kernel, K1r and K1mr, which keep their registers and occupancy -- and the row's third meta word
 * carries sampleBytes / sampleBits per stream, so K2r and KF form block 0 and its CRC as they did.
 * Not covered: following sampleBits from the incoming meta blocks unless sdrhip_rx_set_follow_bits is on (the datagram entries: the
 * followed size then wins over the array wherever it exists), the uniform step and pipelined mode, the Tx pipe.  (The input
 * format per stream -- sdrhip_rx_set_input_format is bank-wide -- is sdrhip_rx_set_stream_format, below.) */
int sdrhip_rx_set_stream_bits(sdrhip_rx *rx, const unsigned *sample_bits);
int sdrhip_rx_get_stream_bits(const sdrhip_rx *rx, int stream, unsigned *sample_bits, unsigned *frame_bits);

/* ---- Per-stream input format: 8- and 16-bit IQ rows in one call.
 * In the reference the format belongs to the source object, which is per process and so per stream: RtlSdrSource.cpp:542-553 makes
 * IQSample(buf[2i] - 128, buf[2i+1] - 128) of its offset-binary bytes, HackRFSource.cpp:661-674 makes IQSample(buf[2i], buf[2i+1])
 * of its signed bytes, the 12- and 16-bit sources deliver int16, and sdrdaemonrx.cpp:264-374 picks one source per process.
 * sdrhip_rx_set_stream_format: fmt = host array of nstreams entries, each SDRHIP_IQ_S16, SDRHIP_IQ_U8 or SDRHIP_IQ_S8; NULL =
 * bank-wide again (the value of sdrhip_rx_set_input_format).  sdrhip_rx_get_stream_format: *fmt = the format in force for the stream.
 * Contract.  Per stream the result is byte for byte that of a one-stream sdrhip_rx with sdrhip_rx_set_input_format(fmt[s]) fed the
 * same bytes, call after call: frames, recovery blocks, meta blocks, frameIndex and all carried state.
 * Sample size: the format implies none.  cfg.sample_bits / sdrhip_rx_set_stream_bits stay the caller's; an RTL-SDR stream sets 8 there.
 * Entries: the setting holds through sdrhip_rx_process_ragged (host and device memory), sdrhip_rx_submit_ragged,
 * sdrhip_rx_collect_ragged and sdrhip_rx_collect_egress, together with the stream meta, fecblk and bits arrays in any combination.
 * While the array is set every step is the ragged step: sdrhip_rx_process, sdrhip_rx_submit and sdrhip_rx_set_pipelined(1) return
 * SDRHIP_EINVAL with nothing consumed.  The datagram entries ignore the array, as they ignore sdrhip_rx_set_input_format: the wire
 * carries IQSample.
 * Addressing while the array is set.  Counts stay in samples.  Strided rows: row s starts at byte 4 * s * in_stride whatever its
 * format; in_stride counts 4-byte units and is at least the largest count; an 8-bit row occupies the first 2 * n_in[s] bytes of its
 * row.  Device memory: base 16-byte aligned, in_stride a multiple of 4; nothing outside a row's n_in[s] * bytes(fmt[s]) bytes is
 * read.  Packed (in_stride = SDRHIP_PACKED, the asynchronous entry): rows back to back in bytes, row s of a block starts at
 * sum_{t<s} n_in[t] * bytes(fmt[t]) -- an int16 row may start 2 bytes off a dword boundary.  An array of equal entries is allowed:
 * with packed input it delivers the bytes of that bank-wide format; with strided input the stride unit is the 4-byte unit above
 * (bank-wide 8-bit strides count 2-byte samples).
 * The setter changes host state only: nothing is enqueued, nothing waited for.  It is refused, nothing changed, for a NULL handle,
 * a value outside the three formats, a pipelined pipe or one with late frames waiting, and while asynchronous batches are being
 * filled or in flight (the rule of sdrhip_rx_set_input_format): a batch has one set of formats.  sdrhip_rx_set_input_format stays
 * allowed; while the array is set its value is unused.  sdrhip_rx_reconfigure and sdrhip_rx_reset_streams do not clear the array;
 * export and import of a stream are untouched (the format is configuration).  A handle on which the setter was never called
 * launches the same kernels in the same order with the same arguments.
 * Link traffic: a ragged batch uploads exactly sum n_in[s] * bytes(fmt[s]) sample bytes ("h2d_bytes").
 * How: K0x (rx_unpack_mixed_kernels.hip) is K0p with the format read from the stream's row of the per-call table and segment
 * sources in 2-byte units; the synchronous call is a K0x launch with one segment per stream, over the staged upload (host memory)
 * or the caller's rows in place (device memory) -- one pass over the int16 rows more than the bank-wide int16 call.
 * Not covered: a per-stream decimation or Fc position, following sampleBits from the incoming meta blocks unless
 * sdrhip_rx_set_follow_bits is on (the datagram entries, which ignore this array).  (The Tx pipe has an output format per stream
 * of its own: sdrhip_tx_set_stream_format, below.) */
int sdrhip_rx_set_stream_format(sdrhip_rx *rx, const int *fmt);
int sdrhip_rx_get_stream_format(const sdrhip_rx *rx, int stream, int *fmt);

/* ---- Per-stream output format of the Tx pipe: HackRF and int16 sinks in one bank.
 * In the reference the format belongs to the sink object, which is per process and so per stream: HackRFSink.cpp:671-672 sends
 * real() >> 8, imag() >> 8, FileSink.cpp:216-277 writes int16 IQ, and sdrdaemontx.cpp:195-255 picks one sink per process.
 * sdrhip_tx_set_stream_format: fmt = host array of nstreams entries, each SDRHIP_IQ_S16 or SDRHIP_IQ_S8; NULL = bank-wide again
 * (the value of sdrhip_tx_set_output_format).  sdrhip_tx_get_stream_format: *fmt = the format in force for the stream.
 * Contract.  Per stream the result is byte for byte that of a one-stream sdrhip_tx with sdrhip_tx_set_output_format(fmt[s]) fed the
 * same input, call after call: samples, meta blocks, records and all carried histories.
 * Entries: the array holds through sdrhip_tx_process (host and device memory), pipelined mode and sdrhip_tx_flush, sdrhip_tx_submit /
 * sdrhip_tx_collect, sdrhip_tx_process_datagrams, sdrhip_tx_submit_datagrams / sdrhip_tx_submit_datagrams_tagged /
 * sdrhip_tx_collect_datagrams.  A batch takes the formats in force when it is handed in, as it takes the factor.
 * Addressing while the array is set (the rule of sdrhip_rx_set_stream_format, mirrored).  Counts stay in samples.  out_stride counts
 * 4-byte units: row s starts at byte 4 * s * out_stride whatever its format; an 8-bit row occupies the first 2 * n bytes of its row,
 * nothing behind them is written.  Device memory: base 16-byte aligned, out_stride a multiple of 4, else SDRHIP_EALIGN.  An array of
 * equal entries is allowed: it gives the bytes of that bank-wide format in the 4-byte stride unit (bank-wide 8-bit strides count
 * 2-byte samples).
 * The setter changes host state only: nothing is enqueued, nothing waited for.  It is refused, nothing changed, for a NULL handle,
 * SDRHIP_IQ_U8 or an unknown value in any entry, while asynchronous batches are in flight and while a pipelined batch waits (the
 * rules of sdrhip_tx_set_output_format).  sdrhip_tx_set_output_format stays allowed; while the array is set its value is unused.
 * sdrhip_tx_reconfigure and sdrhip_tx_reset_streams do not clear the array; export and import of a stream are untouched (the format
 * is configuration): an imported stream takes the destination's format.  The no-copy mode (option tx_gather) does not apply while
 * the array is set.  A handle on which the setter was never called launches the same kernels in the same order with the same
 * arguments.
 * Link traffic: every host-memory entry downloads exactly sum_s n[s] * bytes(fmt[s]) sample bytes, plus records and meta blocks as
 * before ("d2h_bytes").
 * How: K5x (interp_mixed_kernels.hip) is K5 / K5w with one int per stream read by a scalar load and a wave-uniform branch to the
 * int16 or the 8-bit last stage; K6x is x1, a copy or the narrowing per stream.  The table of formats goes up on the context's stream
 * in front of the first launch after a change.
 * Not covered: a per-stream interpolation factor, SDRHIP_IQ_U8 on Tx, a format argument for the bare sdrhip_interpolate. */
int sdrhip_tx_set_stream_format(sdrhip_tx *tx, const int *fmt);
int sdrhip_tx_get_stream_format(const sdrhip_tx *tx, int stream, int *fmt);

/* ---- Per-stream lifecycle: one stream of a bank begins again while the others run on.
 * In the reference one stream is one sdrdaemonrx / sdrdaemontx process, and restarting that process gives the stream what the
 * constructors leave: zero half-band histories (Decimators.h:56-70, Interpolators.h:47-52: EO1.h:171-188 / IntHalfbandFilterDB's
 * zero fill), no open frame and m_frameCount 0 (UDPSinkFEC.cpp:28-60), an SDRdaemonFECBuffer with frame head -1, empty slots,
 * statistics 256 / 0 and MetaDataFEC::init() in m_currentMeta and m_outputMeta (SDRdaemonFECBuffer.cpp:28-52).
 * mask: host array of nstreams bytes, nonzero = reset that stream; NULL = every stream (for the pipes: the whole-pipe reset).
 * Afterwards stream s behaves, byte for byte, like stream s of a freshly created handle with the present configuration; every
 * other stream behaves as if the call had not happened.
 *  - sdrhip_decimators_reset_streams / sdrhip_interpolators_reset_streams: the streams' filter histories.
 *  - sdrhip_fecbuf_reset_streams: the streams' collector state and statistics (and, on an Rx handle's collector, the samples the
 *    stream holds back in front of its decimator: sdrhip_rx_carry reads 0).
 *  - sdrhip_rx_reset_streams: the six decimator histories; the open frame, which is discarded and never delivered (its window
 *    slot may keep stale bytes); m_frameCount, back to 0; with a datagram collector also what sdrhip_fecbuf_reset_streams covers,
 *    so that m_outputMeta reads "no incoming meta" for sdrhip_rx_set_follow_meta until the stream's next block 0 is released.
 *  - sdrhip_tx_reset_streams: the interpolator histories, and the collector if there is one.
 * What survives: the configuration, the sdrhip_rx_set_stream_meta arrays, the two follow flags, the input / output format, the
 * asynchronous ring.
 * Ordering: the call takes the context lock and enqueues ONE small launch on the context's stream behind everything submitted so
 * far; it never synchronises and reads nothing back (the mask goes up from a pinned version of its own: a launch in flight never
 * sees a later call's mask; an all-zero mask launches nothing).  On a collector whose host shadow is valid the host writes the
 * constructor's values into the shadow itself: the next sdrhip_*_submit_datagrams still reads nothing back.  Allowed between any
 * two calls, also between two submits while batches are in flight: those keep what they were enqueued with.  After a partial
 * sdrhip_rx_reset_streams the streams stand at different frame positions: sdrhip_rx_process takes its ragged step, and
 * sdrhip_rx_set_pipelined(1) / sdrhip_rx_submit refuse as they do after ragged calls (a pipe that IS pipelined cannot take the
 * ragged step: leave pipelined mode, or reset the whole pipe, before the next sdrhip_rx_process).  A reset of EVERY stream (NULL,
 * or a mask that names them all) also puts every stream's frame window back to the start of the frame area, whatever ragged
 * calls moved the windows apart before: the streams stand at the same position again, and the uniform step, pipelined mode and
 * uniform batches are available as on a fresh handle.
 * SDRHIP_EINVAL, nothing changed: a NULL handle; on a pipe, a uniform or ragged batch that is being filled (collect it first), and
 * frames or a batch of a pipelined pipe that wait for delivery (sdrhip_*_flush first).
 * A handle on which none of these was called launches exactly what it launched before they existed. */
int sdrhip_decimators_reset_streams(sdrhip_decimators *d, const uint8_t *mask);
int sdrhip_interpolators_reset_streams(sdrhip_interpolators *p, const uint8_t *mask);
int sdrhip_fecbuf_reset_streams(sdrhip_fecbuf *b, const uint8_t *mask);
int sdrhip_rx_reset_streams(sdrhip_rx *rx, const uint8_t *mask);
int sdrhip_tx_reset_streams(sdrhip_tx *tx, const uint8_t *mask);
/* Export and import of ONE stream: what carries a live stream from one bank to another (a hub rebalancing "stream s on rank
 * s mod N", a process replaced without a glitch), the way a checkpointed sdrdaemonrx / sdrdaemontx would be carried.
 * The blob is host memory, opaque, sdrhip_*_stream_state_bytes() long: fixed per kind, independent of the configuration (0 for a
 * NULL handle).  It starts with a 16-byte header {magic "SDRS", version 1, kind 1 = rx / 2 = tx, total bytes}.  An Rx blob holds
 * hb_variant; the stream's decimator row (the six histories of Decimators.h:56-70) and whether its first-stage history fits int16;
 * r_pending, r_open and r_count (UDPSinkFEC's sample index, open frame and m_frameCount); the 128 super blocks of the open frame with
 * the meta block it was opened with (UDPSinkFEC.cpp:160-165); a "has collector" flag and, with a collector, the stream's
 * SDRdaemonFECBuffer state, the 128 super blocks of its current carry buffer, and its held-back samples (at most 63) with their
 * count.  A Tx blob holds the interpolator row (Interpolators.h:47-52) and the same collector part.  What a stream does not have
 * is zero -- no open frame, no collector, the carry buffer's rows the open slot has not filled yet, the sample slots behind the
 * held-back count --: a just-reset stream's blob equals a never-used stream's, byte for byte.
 * Export leaves the source untouched; it synchronises once (one gather launch, one copy of the packed bytes, one wait).
 * Import makes stream `stream` of the destination -- any Rx or Tx bank, on any context, of any nstreams -- continue exactly where
 * the source stream stood: it enqueues ONE upload and ONE scatter launch on the context's stream and does not synchronise (the
 * upload is staged in the next of four pinned buffers of the handle: only a fifth import in a row waits, for the upload of the
 * first; the
 * first import that must create the bank's collector, its rows or its frame area allocates them, as a first call does).  The
 * destination's own log2decim, fcpos, nb_fec, meta arrays and log2interp apply from then on, as after sdrhip_*_reconfigure: the open
 * frame keeps its meta block and is encoded with the fecblk in force when it completes.  A blob without a collector leaves the
 * stream of a bank that has one with the constructor's collector state.  Import clears the bank-wide "first-stage history fits
 * int16" shortcut when the blob says so, and patches a valid collector shadow as the reset does.  The other streams of both banks
 * run on undisturbed.  An imported stream stands at its own frame position, as a stream does after a partial
 * sdrhip_rx_reset_streams: unless that position is the other streams' too, sdrhip_rx_process takes its ragged step from then on, and
 * sdrhip_rx_set_pipelined(1) / sdrhip_rx_submit refuse with SDRHIP_EINVAL, nothing consumed, until a reset of every stream.
 * SDRHIP_EINVAL, nothing changed: a NULL handle or blob; a wrong size, magic, version or kind; a blob of another hb_variant; a
 * stream outside the bank; a blob whose fields no stream can be in; any asynchronous batch being filled or in flight; a
 * pipelined pipe with frames or a batch waiting (flush first).
 * A handle on which none of these was called launches exactly what it launched before they existed. */
size_t sdrhip_rx_stream_state_bytes(const sdrhip_rx *rx);
size_t sdrhip_tx_stream_state_bytes(const sdrhip_tx *tx);
int sdrhip_rx_export_stream(sdrhip_rx *rx, int stream, void *blob, size_t bytes);
int sdrhip_rx_import_stream(sdrhip_rx *rx, int stream, const void *blob, size_t bytes);
int sdrhip_tx_export_stream(sdrhip_tx *tx, int stream, void *blob, size_t bytes);
int sdrhip_tx_import_stream(sdrhip_tx *tx, int stream, const void *blob, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SDRHIP_H */
