/*
 * amr.h -- C ABI of libamr.so, the MI355X (gfx950) batched demodulator core.
 *
 * Plain C: pointers, sizes and status codes only.  Host-side callers are the
 * drop-in Python modules in audio-modem-radio_amd/ (ctypes; INTEGRATION.md
 * shows the binding) and bench.py.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to szumanski/Audio-Modem-Radio):
 *
 *   amr_psk_plan_create     the per-call filter/LO setup inside
 *                           modem.qpsk_demodulate   modem.py:191-204
 *                           modem.bpsk_demodulate   modem.py:70-88
 *                           (the host designs b/a/zi with scipy exactly like
 *                            the reference and hands them over; the LO table
 *                            is numpy's exp(-1j*2*pi*fc*t), modem.py:82,201)
 *   amr_psk_demod_host      modem.qpsk_demodulate(samples, baud, carrier, fs)
 *                           modem.py:189-266 (also psk8_demodulate modem.py:348,
 *                           ofdm_demodulate_simple modem.py:375-376, and the
 *                           decoder dispatch decoder.py:422-434) and
 *                           modem.bpsk_demodulate modem.py:68-135 -- for a whole
 *                           batch of equal-length streams per call
 *   amr_psk_demod_device    the same with the batch already resident in HBM
 *   amr_psk_demod_host_edges  the same for a raw-integer / float16 array, whose
 *                           odd extension scipy forms in that dtype (modem.py:198, 77)
 *   amr_psk_demod_fec_device  8PSK alias + fec.ReedSolomonFEC.decode fused
 *                           (modem.py:348 then fec.py:34-69; BASELINE config 5)
 *   amr_fsk_plan_create     the per-call butter/lfilter_zi setup of
 *                           modem.fsk_demodulate    modem.py:301-307
 *   amr_fsk_demod_host      modem.fsk_demodulate    modem.py:298-341 (also
 *                           fsk_high_speed_demodulate modem.py:355-356,
 *                           ft8_demodulate modem.py:391), batched
 *   amr_fsk_envelopes_host  the envelopes |hilbert(filtfilt(.))| modem.py:308-309
 *   amr_hilbert_host        scipy.signal.hilbert as modem.py:309 calls it
 *   amr_resample_host       scipy.signal.resample in decode_wav_file decoder.py:385-387
 *   amr_fec_decode_host     fec.ReedSolomonFEC.decode  fec.py:34-69, batched
 *   amr_frame_parse_host    decoder.parse_fbp_stream_enhanced  decoder.py:142-208,
 *                           batched (magic search, checks, payload CRC32)
 *   amr_modulate_host       modem.bpsk_modulate / qpsk_modulate / fsk_modulate
 *                           (modem.py:28-65, 138-186, 270-295) + the int16 of
 *                           wav_from_array (modem.py:360-368), batched
 *   amr_hell_demod_host     hellschreiber.hellschreiber_demodulate
 *                           (hellschreiber.py:155-187), batched; AMR_TX_HELL is
 *                           hellschreiber_modulate (hellschreiber.py:109-152)
 *   amr_conv_encode_host    fec.ConvolutionalEncoder.encode  fec.py:79-111, batched
 *   amr_viterbi_decode_host the maximum-likelihood decoder of that code, batched
 *                           (no reference counterpart: fec.ViterbiDecoder.decode,
 *                           fec.py:126-155, is a stub and stays one in fec.py)
 *   amr_rs_encode_host      fec.ReedSolomonCodec: systematic RS(255, 255 - nsym) over
 *   amr_rs_decode_host      GF(2^8), errors-and-erasures decoding, block interleave
 *                           (no reference counterpart: fec.ReedSolomonFEC is parity)
 *   amr_allgather           the gather of decoded bytes across GPUs (RCCL)
 *
 * Status: every function returns AMR_OK (0) or a negative AMR_E_* code;
 * amr_last_error() gives the message of the calling thread's last failure.
 * Ownership: host buffers are borrowed for the duration of a synchronous
 * call; device buffers passed to *_device calls must stay valid until the
 * plan's stream is synchronised (amr_psk_plan_synchronize).  A plan owns its
 * device scratch; calls on one plan are serialised by a per-plan mutex, so
 * two host threads may share a plan (the reference decodes from a capture
 * QThread and the GUI thread, filebeep_advanced_v2.py:324,1112).
 */
#ifndef AMR_H
#define AMR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMR_ABI_VERSION 5   /* 2: AMR_TF_EXACT (AMR_TF_COUNT 5), amr_fsk_plan_exact_streams / _set_exact_mode,
                                 amr_resample_host bit-exact; size timing arrays from AMR_*_COUNT
                               3: AMR_LAYOUT_SPLIT, amr_psk_plan_set_layout, amr_psk_plan_split_info,
                                  amr_psk_split_design, amr_psk_split_symbols_host, the float32 hand-off
                                  (amr_psk_f32_margin, amr_psk_plan_last_f32f), amr_fsk_plan_resident_bytes,
                                  the FSK time-split F1 (AMR_FSK_LAYOUT_*, amr_fsk_plan_set_layout,
                                  amr_fsk_plan_split_info, amr_fsk_split_design, amr_fsk_split_bandpass_host)
                               4: the time-split passes' chunk start states by convolution
                                  (amr_split_state_tables, amr_psk_plan_split_conv, amr_fsk_plan_split_conv)
                               5: raw-integer captures: amr_psk_demod_host_edges / _device_edges,
                                  amr_fsk_demod_host_edges / _device_edges (the odd extension as the
                                  caller's dtype forms it); the PSK split's strict mode
                                  (amr_psk_plan_set_split_strict ...); F2's margin from a standard
                                  FFT rounding bound (amr_fsk_fft_margin, amr_fsk_plan_margin); the FSK
                                  split's strict mode (amr_fsk_plan_set_split_strict ...)
                                  additions under 5 (nothing existing changed): the Hellschreiber
                                  receiver (amr_hell_pixels, amr_hell_work_bytes, amr_hell_demod_host /
                                  _device, amr_hell_glyph_rows, AMR_HELL_ELEM_*) and AMR_TX_HELL; the
                                  convolutional code (amr_conv_encoded_len, amr_conv_encode_host,
                                  amr_viterbi_work_bytes, amr_viterbi_decode_host / _device);
                                  amr_psk_plan_last_lowpass (AMR_LP_*); amr_sync_pack_host (diagnostic);
                                  the Reed-Solomon code (amr_rs_encoded_len, amr_rs_decoded_len,
                                  amr_rs_encode_host / _device, amr_rs_decode_host / _device);
                                  the 8-ary differential PSK modem: AMR_PSK_D8PSK (a plan kind,
                                  and a kind of amr_psk_slice_host / amr_psk_soft_host) and
                                  AMR_TX_D8PSK (a modulation mode); the multi-carrier DQPSK
                                  modem (amr_ofdm_*, AMR_TO_*); the direct-sequence DBPSK
                                  modem (amr_dsss_*, AMR_TD_*); the two-ring 16-DAPSK modem
                                  star16: AMR_PSK_STAR16 (a plan kind, and a kind of
                                  amr_psk_slice_host / amr_psk_soft_host) and AMR_TX_STAR16
                                  (a modulation mode) */

#define AMR_OK 0
#define AMR_E_INVALID -1      /* bad argument */
#define AMR_E_PADLEN -2       /* n_samples <= filtfilt padlen (scipy ValueError) */
#define AMR_E_HIP -3          /* HIP runtime failure (message in amr_last_error) */
#define AMR_E_NOMEM -4        /* device allocation failed */
#define AMR_E_NODEVICE -5     /* no usable gfx950 device */
#define AMR_E_RCCL -6         /* RCCL failure */
#define AMR_E_CAPACITY -7     /* batch larger than the plan's max_streams */

#define AMR_DTYPE_F32 0       /* float32 samples (live capture path) */
#define AMR_DTYPE_F64 1       /* float64 samples (decode_wav_file path) */
#define AMR_DTYPE_I16 2       /* int16 PCM, read as int16/32768.0 (libsndfile default) */

#define AMR_PSK_QPSK 0        /* DQPSK slicer, modem.py:216-241 */
#define AMR_PSK_BPSK 1        /* DBPSK slicer, modem.py:102-105 */
/* d8psk: 8-ary differential PSK, 3 bits per symbol (no reference counterpart:
 * the reference's "8PSK" is a QPSK alias).  QPSK's filters,
 * sps and first symbol; on d = s[k+1] * conj(s[k]) (numpy's multiply), with
 * T = 0x1.a827999fcef32p-2 (tan(pi/8)), ar = |dr|, ai = |di|:
 *   ai < T*ar: m = dr > 0 ? 0 : 4;  else ar < T*ai: m = di > 0 ? 2 : 6;
 *   else m = di > 0 ? (dr > 0 ? 1 : 3) : (dr > 0 ? 7 : 5)
 * and the bits are the Gray code m ^ (m >> 1), MSB first, 3 (S - 1) per stream
 * in one contiguous string; sync search and byte pack as for the others.  A
 * d8psk plan never runs the time-split layout (it takes the row layout
 * instead) and its lane layout always slices in a kernel of its own. */
#define AMR_PSK_D8PSK 2
/* star16: two-ring 16-ary differential amplitude and phase keying, 4 bits per
 * symbol (a, b2, b1, b0) (no reference counterpart: the reference's "APSK16"
 * is a QPSK alias).  QPSK's filters, sps and first symbol.
 * b2 b1 b0 is d8psk's tribit of d = s[k+1] * conj(s[k]), unchanged.  With
 * e = sr*sr + si*si of a symbol (two rounded products, one rounded sum):
 *   a = (e[k+1] > 2.0 * e[k]) | (e[k] > 2.0 * e[k+1])      (the ring changed)
 * -- false for NaN, inf against inf, zeros and exact ties.  The nibble 8 a + g
 * goes out MSB first, 4 (S - 1) bits per stream, eight products per word; sync
 * search and byte pack as for the others.  Soft values (amr_psk_demod_soft_*,
 * amr_psk_soft_host): four per product, a's magnitude from
 *   num = min(|e1 - 2.0 e0|, |e0 - 2.0 e1|), den = e0 + e1
 * by the common rule, the other three d8psk's.  Both decisions compare like
 * with like: a capture scaled by any power of two decodes to the same bits.
 * As d8psk, a star16 plan never runs the time-split layout (it takes the row
 * layout instead) and its lane layout always slices in a kernel of its own.
 * (Kind 3 is not assigned.) */
#define AMR_PSK_STAR16 4

/* kernel timing slots reported by amr_psk_plan_timings() */
#define AMR_T_BANDPASS 0
#define AMR_T_LOWPASS_FWD 1
#define AMR_T_LOWPASS_BWD 2
#define AMR_T_LOWPASS_EXACT 3
#define AMR_T_SYNC_PACK 4
#define AMR_T_FEC 5
#define AMR_T_LAUNCH 6     /* the whole launch: first kernel start -> last output written, or, when the
                            * launch's outputs are all-gathered (amr_allgather with this plan), -> gathered */
#define AMR_T_COUNT 7

typedef struct amr_psk_plan amr_psk_plan;
typedef struct amr_comm amr_comm;

int amr_abi_version(void);
/* sha256 prefix of the sources this library was built from (build.py
 * source_hash): ties a loaded binary to the tree's sources */
const char *amr_build_id(void);
const char *amr_last_error(void);
int amr_device_count(int *count);

/* ---- memory helpers (device = the plan's / current device) ---------------- */
int amr_set_device(int device);
int amr_malloc(void **dptr, int64_t bytes);
int amr_free(void *dptr);
int amr_memcpy_h2d(void *dst, const void *src, int64_t bytes);
int amr_memcpy_d2h(void *dst, const void *src, int64_t bytes);
int amr_memcpy_d2d(void *dst, const void *src, int64_t bytes);
int amr_device_synchronize(void);

/* ---- DPSK demodulation ------------------------------------------------------
 * kind          AMR_PSK_QPSK | AMR_PSK_BPSK | AMR_PSK_D8PSK | AMR_PSK_STAR16
 * n_samples     samples per stream (all streams of a call share it)
 * sps           int(fs / baud)                                 modem.py:70,191
 * first_symbol  sps // 2 (QPSK, modem.py:209; d8psk, star16) or sps (BPSK, modem.py:92)
 * bp_*          band-pass b, a, lfilter_zi (ntaps each; a[0] must be 1)
 * lp_*          low-pass  b, a, lfilter_zi
 * lo4           [n_samples][4] doubles: lo_re, lo_im, -(0*lo_im), 0*lo_re
 *               where lo = numpy.exp(-1j*2*pi*carrier*arange(n)/fs)
 * max_streams   largest batch this plan will see (sizes the HBM scratch)
 */
int amr_psk_plan_create(amr_psk_plan **plan, int device, int kind, int64_t n_samples, int64_t sps,
                        int64_t first_symbol, const double *bp_b, const double *bp_a, const double *bp_zi,
                        int bp_ntaps, const double *lp_b, const double *lp_a, const double *lp_zi,
                        int lp_ntaps, const double *lo4, int64_t max_streams);
int amr_psk_plan_destroy(amr_psk_plan *plan);
/* bytes a stream's output can need: floor(bits/8) */
int64_t amr_psk_plan_out_capacity(const amr_psk_plan *plan);
/* the most device memory the plan can hold: scratch (its row-layout buffers
 * are allocated on the first call that runs that layout) + the host-API
 * staging (allocated on the first amr_psk_demod_host call) */
int64_t amr_psk_plan_scratch_bytes(const amr_psk_plan *plan);
/* the amr_psk_plan_scratch_bytes a plan of this shape would report, without
 * creating it (the drop-in plan cache evicts for it first); < 0 on bad args */
int64_t amr_psk_plan_bytes_estimate(int kind, int64_t n_samples, int64_t sps, int64_t first, int bp_ntaps,
                                    int lp_ntaps, int64_t max_streams);
int amr_psk_plan_synchronize(amr_psk_plan *plan);
/* record per-kernel HIP events on the plan's stream (1) or not (0) */
int amr_psk_plan_enable_timing(amr_psk_plan *plan, int on);
/* hint: the caller keeps `batches` batches in flight at once, each on its own
 * plan (stream); the band-pass layout is then chosen for n_streams x batches
 * concurrent streams.  Default 1.  No reference counterpart:
 * a batching knob of this build (the reference decodes one stream per call,
 * decoder.py:417-464). */
int amr_psk_plan_set_inflight(amr_psk_plan *plan, int batches);
/* milliseconds of each AMR_T_* kernel in the last call (-1 = not run) */
int amr_psk_plan_timings(amr_psk_plan *plan, float *ms, int count);
/* kernel layout of the last call: AMR_LAYOUT_ROW = states spread over lanes
 * (psk_kernels.hip), AMR_LAYOUT_LANE = one stream per lane
 * (psk_lane_kernels.hip), AMR_LAYOUT_SPLIT = each filtfilt pass cut in time
 * into chunks, decisions kept where a margin proves them the reference's and
 * a batch with any other stream re-run by the row kernels
 * (psk_split_kernels.hip).  Picked by streams in flight
 * (DESIGN.md §3): split for <= 64 (one capture at a time, as the reference's
 * own callers decode -- filebeep_advanced_v2.py:324, 1112), row up to
 * 16383, lane from 16384. */
#define AMR_LAYOUT_ROW 0
#define AMR_LAYOUT_LANE 1
#define AMR_LAYOUT_SPLIT 2
int amr_psk_plan_last_layout(const amr_psk_plan *plan);
/* force a layout for this plan's calls (-1: by streams in flight, the
 * default).  No reference counterpart: a test / tuning knob; the bytes are
 * the reference's in every layout. */
int amr_psk_plan_set_layout(amr_psk_plan *plan, int layout);
/* the time-split layout of this plan: streams its last call flagged for the
 * serial path (-1 when that call ran another layout; synchronises the plan's
 * stream), the band-pass / low-pass warm-up samples and the symbols' error
 * bound per unit input peak (-1 when the plan's filters do not allow the
 * layout), and the last call's chunk length (0 before any).  Any pointer may
 * be NULL. */
int amr_psk_plan_split_info(amr_psk_plan *plan, int64_t *flagged, int64_t *warmup_bp, int64_t *warmup_lp,
                            int64_t *chunk, double *kappa);
/* The time-split design of a band-pass / low-pass pair (host arithmetic, no
 * device): warm-up samples per filter and kappa, the bound on a symbol
 * sample's error per unit input peak; AMR_E_INVALID when the
 * filters do not allow the layout (warm-ups over n / 4, not 9 + 5 taps). */
int amr_psk_split_design(const double *bp_b, const double *bp_a, int bp_ntaps, const double *lp_b,
                         const double *lp_a, int lp_ntaps, int64_t n_samples, int64_t n_sym, int64_t *warmup_bp,
                         int64_t *warmup_lp, double *kappa);
/* The lane layout's float32 hand-off: the bound on a symbol
 * sample's error per unit of the stream's max |band-pass output| when the
 * low-pass reads that output rounded to float32 (host arithmetic on the
 * low-pass b, a; 0: no hand-off for these coefficients), and whether the
 * plan's last call used the hand-off (1) or float64 (0). */
double amr_psk_f32_margin(const double *lp_b, const double *lp_a, int lp_ntaps);
int amr_psk_plan_last_f32f(const amr_psk_plan *plan);
/* Diagnostic (tests, A/B runs): which low-pass kernel the plan's last call ran
 * in the lane layout -- AMR_LP_LANE: k_lp_lane, symbols to
 * HBM for the slicer kernel; AMR_LP_LANE_FUSED: k_lp_lane with the
 * slicer fused, a component per wave; AMR_LP_LANE_HALF: k_lp_lane_h, both
 * components in one wave, the slicer inline -- or -1 when that call ran no
 * lane low-pass (another layout, or every stream through the exact path). */
#define AMR_LP_LANE 0
#define AMR_LP_LANE_FUSED 1
#define AMR_LP_LANE_HALF 2
int amr_psk_plan_last_lowpass(const amr_psk_plan *plan);
/* Diagnostic (tests): the time-split passes alone over a host batch, chunk
 * outputs per lane (0: the plan's rule) -> the symbol samples
 * sym [n_streams][n_sym][re, im] (baseband[first::sps], modem.py:92, 209, as
 * the time-split layout computes them -- not bit-exact).
 * With the convolution chunk starts on, a chunk in 1..127 is refused
 * (AMR_E_INVALID): the start states take n_streams x m1 / chunk x 64 B. */
int amr_psk_split_symbols_host(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                               int64_t chunk, double *sym);
/* The time-split band-pass's chunk start states: instead of
 * running w samples of recursion from a zero state, a chunk starting at
 * output t0 takes Z0[t0] v0 + sum_{m < min(t0, w)} K[m] v(t0 - 1 - m) (the
 * Z0 term while t0 <= w), a dot product the GPU spreads over a wave.  Host
 * arithmetic (long double, rounded once) for a DF-II-T filter b, a (a[0] = 1,
 * ntaps - 1 states) and scipy's zi: K [w][ntaps - 1] = the state after a unit
 * input and m zero inputs, Z0 [w + 1][ntaps - 1] = zi after t zero inputs.
 * amr_psk_plan_split_conv: 1 when the plan's time-split layout uses them (its
 * tables are built with the design; AMR_PSK_SPLIT_CONV=0 selects the
 * warm-ups), 0 when not, -1 for NULL.  Both replace no reference function
 * (modem.py:194-199's filtfilt is what they approximate). */
int amr_split_state_tables(const double *b, const double *a, const double *zi, int ntaps, int64_t w, double *K,
                           double *Z0);
int amr_psk_plan_split_conv(amr_psk_plan *plan);
/* The time-split layout's STRICT mode (csrc/split_strict.h).
 * By default a split decision is kept when it clears kappa * peak|x| -- a
 * measured premise (the worst error over the test signal classes and the
 * adversarial search is >= 54x below it), not a bound.  Strict mode keeps it
 * only when it clears a bound that holds for every input: per-step rounding
 * bounds and chunk-start error bounds the kernels measure on the stream itself,
 * carried through the filters' L1 response gains to a bound per symbol; a
 * decision inside it goes to the serial row kernels as before.  Bytes are the
 * reference's in both modes wherever the premise holds; strict mode makes
 * that unconditional at the cost of more flagged captures.
 * amr_psk_plan_set_split_strict: 1 on, 0 off, -1 the process default
 * (AMR_PSK_SPLIT_STRICT=1 turns it on); amr_psk_plan_split_strict: whether this
 * plan's split calls use it; amr_psk_plan_last_strict: whether the last split
 * call did.  No reference counterpart (modem.py:197-214 is what is bounded). */
int amr_psk_plan_set_split_strict(amr_psk_plan *plan, int mode);
int amr_psk_plan_split_strict(amr_psk_plan *plan);
int amr_psk_plan_last_strict(const amr_psk_plan *plan);
/* Diagnostic (tests): the strict passes over a host batch -> the symbol
 * samples sym [n_streams][n_sym][re, im], the bound e [n_streams][n_sym] on
 * each symbol component's |split - reference| and, per stream, scalars
 * [n_streams][4]: E1 (band-pass forward), F (band-pass output), X (mixer
 * output) and P3 (low-pass input peak; negative when the a-posteriori caps
 * failed and the stream would be flagged).  A plan without decision bits
 * (fewer than two symbol centres) is refused, AMR_E_INVALID, and nothing is
 * written.  (amr_psk_split_symbols_host with an explicit chunk runs that
 * chunk as given, without the strict bookkeeping, whatever the plan's mode.) */
int amr_psk_split_bounds_host(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                              double *sym, double *ebound, double *scalars);
/* The strict design from the filters alone (host arithmetic; the tests'
 * restatement of the bound uses it): consts[32] = g1x, gmax, hz, tk, zi_sum,
 * zb, kx, ky, u2, gam, c3, w1, w2, n_sym, and the sizes nw, nk, nh, ng, nz,
 * k12_off, the cut remainders w_tail, k12_tail, hs_tail, tz_tail, lp_tail,
 * lp_rad, ok, kappa; tabs (NULL: not written) = kabs [w1] | z0abs [w1 + 1] |
 * lpc [n_sym] | W [nw] | K12 [nk] | HS [nh] | GS [ng] | TZ [nz]. */
int amr_psk_split_strict_design(const double *bp_b, const double *bp_a, const double *bp_zi, int bp_ntaps,
                                const double *lp_b, const double *lp_a, const double *lp_zi, int lp_ntaps,
                                int64_t n_samples, int64_t first, int64_t sps, double *consts, double *tabs);
/* number of streams the exact complex low-pass path re-ran in the last call
 * (time-split layout: 0 when no stream was flagged -- the gated row kernels
 * did not run -- else the flagged streams of the row fallback's low-pass) */
int amr_psk_plan_exact_streams(amr_psk_plan *plan, int64_t *count);

/* x: [n_streams][x_stride] samples of `dtype`; out: [n_streams][out_stride]
 * bytes; out_len[s] = bytes written for stream s; sync_idx[s] = bit index of
 * the "FB" sync or -1.  Synchronous. */
int amr_psk_demod_host(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                       uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx);
/* Same contract, all pointers device pointers; asynchronous on the plan's stream. */
int amr_psk_demod_device(amr_psk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx);
/* Raw-integer captures (ABI 5).  qpsk_demodulate / bpsk_demodulate
 * (modem.py:189-266 / 68-135) hand the caller's array straight to
 * scipy.signal.filtfilt (modem.py:198 / 77), which forms its odd extension
 * 2*x[0] - x[k] (scipy _arraytools.odd_ext, padlen = 3 * bp_ntaps) in the
 * ARRAY's dtype: an int16 capture with |x[0]| > 16383 wraps, uint8 wraps below
 * zero, float16 rounds to half.  A caller with such an array passes the
 * samples converted exactly to AMR_DTYPE_F32 / F64 (their values, not PCM
 * scaling) and the extension as its dtype formed it, in float64:
 *   edges [n_streams][2 * pad]   pad = 3 * bp_ntaps of amr_psk_plan_create
 *   edges[s][j]       = ext index j,           j < pad:  2*x[0] - x[pad - j]
 *   edges[s][pad + r] = ext index pad + n + r, r < pad:  2*x[n-1] - x[n-2-r]
 * (the drop-in builds it with numpy itself, audio-modem-radio_amd/modem.py
 * _raw_input).  Every layout reads the table in place of forming the
 * extension; otherwise as amr_psk_demod_host / _device. */
int amr_psk_demod_host_edges(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             const double *edges, uint8_t *out, int64_t out_stride, int64_t *out_len,
                             int64_t *sync_idx);
int amr_psk_demod_device_edges(amr_psk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                               const double *d_edges, uint8_t *d_out, int64_t out_stride, int64_t *d_out_len,
                               int64_t *d_sync_idx);
/* qpsk_demodulate / bpsk_demodulate (modem.py:189-266 / 68-135) for a batch,
 * as amr_psk_demod_host, queued on the plan's stream (upload, demod, download)
 * without waiting -- the live-capture loop (filebeep_advanced_v2.py:306-324); the host buffers must stay untouched until amr_psk_plan_synchronize.
 * With two or more plans used in turn, batch k+1's upload overlaps batch k's
 * demod (a stream of batches runs at the PCIe rate).  Page-locked buffers
 * (amr_host_register) make the copies fully asynchronous. */
int amr_psk_demod_host_async(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx);
/* (no reference counterpart: the reference's capture buffers are numpy
 * arrays, sounddevice's callback at filebeep_advanced_v2.py:306)
 * page-locked host memory for capture buffers (hipHostMalloc: the full PCIe
 * rate, 57.6 GB/s measured on the MI355X box, against 38 GB/s for a
 * registered pageable buffer) */
int amr_host_alloc(void **ptr, int64_t bytes);
int amr_host_free(void *ptr);
/* page-lock / release a caller's existing host buffer (hipHostRegister) */
int amr_host_register(void *ptr, int64_t bytes);
int amr_host_unregister(void *ptr);
/* Demod then FEC decode of each stream's bytes, fused on the device. */
int amr_psk_demod_fec_device(amr_psk_plan *plan, const void *d_x, int dtype, int64_t n_streams,
                             int64_t x_stride, uint8_t *d_out, int64_t out_stride, int64_t *d_out_len,
                             int64_t *d_sync_idx, uint8_t *d_fec, int64_t fec_stride, int64_t *d_fec_len,
                             int32_t *d_crc_ok);

/* The slicer stage alone (K4a): differential product s[k+1]*conj(s[k])
 * (modem.py:214 / 100) and the QPSK sector / BPSK sign decision
 * (modem.py:216-241 / 102-105) of sym [n_streams][n_sym] complex doubles
 * (re, im interleaved) -> words [n_streams][ceil(bits/32)], bits MSB first,
 * bits = (n_sym-1)*2 (QPSK) or n_sym-1 (BPSK).  Synchronous, current device.
 * For testing the decision at sector edges directly. */
int amr_psk_slice_host(int kind, const double *sym, int64_t n_streams, int64_t n_sym, uint32_t *words);

/* The stage after the slicer alone: the first "0100011001000010" in each
 * stream's n_bits decided bits (bit_str.find, modem.py:247-248) and the whole
 * bytes from there, or from bit 0 without one (modem.py:250-264), MSB first.
 * words [n_streams][n_words], bits MSB first, n_words >= ceil(n_bits/32); bits
 * past n_bits and words past ceil(n_bits/32) are never looked at.  out
 * [n_streams][out_stride], out_stride >= n_bits/8: out_len[s] bytes of row s
 * are written and every other byte of out is returned as it was passed in.
 * sync_idx[s] is the bit index of the sync, -1 without one.  AMR_E_INVALID for
 * a null pointer, a negative count or one of the two sizes too small, before
 * any device work.  Synchronous, current device.  A diagnostic entry like
 * amr_psk_slice_host: for testing the search and the packer at every length
 * and offset directly. */
int amr_sync_pack_host(const uint32_t *words, int64_t n_streams, int64_t n_words, int64_t n_bits, uint8_t *out,
                       int64_t out_stride, int64_t *out_len, int64_t *sync_idx);

/* ---- FSK demodulation (modem.py:298-341) ------------------------------------
 * Replaces modem.fsk_demodulate(samples, baud, mark, space, fs) for a batch of
 * equal-length streams (also fsk_high_speed_demodulate modem.py:355-356,
 * ft8_demodulate modem.py:391 and the decoder's FSK dispatch decoder.py:426-432).
 * n_samples     samples per stream
 * sps           int(fs / baud)                                  modem.py:301
 * mark_* space_* butter(3, [(f-baud)/nyq, (f+baud)/nyq], 'band') b, a and
 *               lfilter_zi (ntaps each, a[0] == 1)              modem.py:307
 * The envelopes |hilbert(filtfilt(...))| (modem.py:308-309) use a double-precision
 * FFT of length n_samples (mixed radix 2/3/4/5, Bluestein otherwise); a stream
 * with a compare the two envelopes' rounding could flip is recomputed exactly
 * (scipy's filtfilt order, pocketfft's transforms), so the decided bytes are
 * the reference's at every length.
 */
#define AMR_TF_BANDPASS 0     /* both tones' filtfilt */
#define AMR_TF_HILBERT 1      /* FFT, -i*sgn(k), inverse FFT, both envelopes and the compare */
#define AMR_TF_DECIDE 2       /* window majority, sync and pack */
#define AMR_TF_LAUNCH 3       /* the whole launch (-> gathered with amr_fsk_allgather), as AMR_T_LAUNCH */
#define AMR_TF_EXACT 4        /* the exact path over the streams F2 flagged (list, filtfilt, envelopes, bits) */
#define AMR_TF_COUNT 5

typedef struct amr_fsk_plan amr_fsk_plan;

int amr_fsk_plan_create(amr_fsk_plan **plan, int device, int64_t n_samples, int64_t sps, const double *mark_b,
                        const double *mark_a, const double *mark_zi, const double *space_b, const double *space_a,
                        const double *space_zi, int ntaps, int64_t max_streams);
int amr_fsk_plan_destroy(amr_fsk_plan *plan);
int64_t amr_fsk_plan_out_capacity(const amr_fsk_plan *plan);
int64_t amr_fsk_plan_scratch_bytes(const amr_fsk_plan *plan);
/* device bytes the plan holds now: scratch_bytes less what the host entries
   allocate on their first call (input / output staging; on a live-layout plan
   the buffer that keeps z through F2) -- a device-entry-only plan's footprint */
int64_t amr_fsk_plan_resident_bytes(const amr_fsk_plan *plan);
/* the amr_fsk_plan_scratch_bytes a plan of this shape would report, without creating it */
int64_t amr_fsk_plan_bytes_estimate(int64_t n_samples, int64_t sps, int ntaps, int64_t max_streams);
/* FFT length actually run: n_samples, or the Bluestein length when n is not 5-smooth */
int64_t amr_fsk_plan_fft_length(const amr_fsk_plan *plan);
/* 1: the plan keeps z and the Hilbert filter's intermediates only for the
 * samples fsk_demodulate's decision windows read (modem.py:320-321: the
 * "live" columns of the four-step grid); 0: every sample */
int amr_fsk_plan_live_columns(const amr_fsk_plan *plan);
int amr_fsk_plan_synchronize(amr_fsk_plan *plan);
int amr_fsk_plan_enable_timing(amr_fsk_plan *plan, int on);
/* the exact path: 0 off (the fast path's bits everywhere -- a diagnostic; decided
 * bytes may then differ from the reference where F2 would have flagged), 1 the
 * streams F2 flags (the default), 2 every stream (tests, timing) */
int amr_fsk_plan_set_exact_mode(amr_fsk_plan *plan, int mode);
/* number of streams the exact path recomputed in the last call (synchronises the plan's stream) */
int amr_fsk_plan_exact_streams(amr_fsk_plan *plan, int64_t *count);
/* milliseconds of each AMR_TF_* stage in the last call (-1 = not run) */
int amr_fsk_plan_timings(amr_fsk_plan *plan, float *ms, int count);
/* Same contracts as amr_psk_demod_host / _device. */
int amr_fsk_demod_host(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                       uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx);
int amr_fsk_demod_device(amr_fsk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx);
/* fsk_demodulate's raw-integer captures (modem.py:308 filtfilt on the
 * caller's array): as amr_psk_demod_host_edges, pad = 3 * ntaps of
 * amr_fsk_plan_create (both tones' filters see the same extension).  F2's
 * ambiguity margin then scales with max(peak|x|, peak|edges|). */
int amr_fsk_demod_host_edges(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             const double *edges, uint8_t *out, int64_t out_stride, int64_t *out_len,
                             int64_t *sync_idx);
int amr_fsk_demod_device_edges(amr_fsk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                               const double *d_edges, uint8_t *d_out, int64_t out_stride, int64_t *d_out_len,
                               int64_t *d_sync_idx);
/* fsk_demodulate (modem.py:298-341), queued without waiting: as
 * amr_psk_demod_host_async */
int amr_fsk_demod_host_async(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx);
/* mark_env, space_env: [n_streams][n_samples] doubles, |hilbert(filtfilt(.))|
 * of each tone (modem.py:308-309) -- the intermediate the tolerance tests read. */
int amr_fsk_envelopes_host(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                           double *mark_env, double *space_env);
/* F1's layout per call.  SERIAL: scipy's filtfilt, one recursion per (stream,
 * tone).  SPLIT: each filtfilt pass cut in time into chunks started early from
 * a zero state (the latency path of one capture): its band-pass
 * output is within kappa * peak|ext x| of scipy's, F2 flags every compare
 * within (2^-36 + kappa * ||hilbert kernel||_1) * peak of a tie, and the exact
 * path re-runs the serial F1 for those streams -- decided bytes unchanged.
 * AUTO (the default): SPLIT for calls of at most 1024 streams when the plan's
 * filters allow it (warm-up <= n / 4) and the exact path is on. */
#define AMR_FSK_LAYOUT_AUTO 0
#define AMR_FSK_LAYOUT_SERIAL 1
#define AMR_FSK_LAYOUT_SPLIT 2
/* 1 when the plan's time-split F1 starts its chunks from convolution states
 * (FS0, amr_split_state_tables per tone) rather than warm-ups
 * (AMR_FSK_SPLIT_CONV=0), 0 when not (or no split design), -1 for NULL. */
int amr_fsk_plan_split_conv(amr_fsk_plan *plan);
int amr_fsk_plan_set_layout(amr_fsk_plan *plan, int layout);
/* the last call's F1 (*last_split 1: split) and the plan's split design:
 * warm-up samples, chunk length of the last split call, kappa, and tau (F2's
 * margin scale for split calls).  Any pointer may be NULL; *warmup = -1 when
 * the plan cannot split. */
int amr_fsk_plan_split_info(amr_fsk_plan *plan, int *last_split, int64_t *warmup, int64_t *chunk,
                            double *kappa, double *tau);
/* F2's margin scale tau from a standard FFT rounding bound (DESIGN.md §2 item
 * 6; host arithmetic, no device): out[8] = tau (max(2^-36, the bound)), the
 * fast path's and pocketfft's relative 2-norm transform errors eps_fast /
 * eps_ref, the bound on max ||z||_2 / peak|ext x| over both tones, whether
 * the fast path runs Bluestein and its length, whether pocketfft does and its
 * length.  The filters as amr_fsk_plan_create takes them.  AMR_E_INVALID
 * when there is no bound: a band-pass whose responses have not decayed within
 * the 4 000 000 steps walked, or grow.  A plan of such filters is still
 * created (amr_fsk_plan_margin then reports tau = +inf) and sends every
 * stream through the exact path, as exact mode 2 does. */
int amr_fsk_fft_margin(int64_t n_samples, const double *mark_b, const double *mark_a, const double *mark_zi,
                       const double *space_b, const double *space_a, const double *space_zi, int ntaps, double *out);
/* a plan's F2 margin scales: tau (serial F1) and tau_split (time-split F1:
 * tau + kappa ||ifft(h)||_1) */
int amr_fsk_plan_margin(amr_fsk_plan *plan, double *tau, double *tau_split);
/* the split design from the filters alone (host arithmetic; no device):
 * warm-up, kappa and ||ifft(h)||_1 of scipy.signal.hilbert's multiplier h at
 * length n.  Returns AMR_E_INVALID when the filters cannot be split at n. */
int amr_fsk_split_design(int64_t n_samples, const double *mark_b, const double *mark_a, const double *space_b,
                         const double *space_a, int ntaps, int64_t *warmup, double *kappa, double *hilbert_l1);
/* The FSK split F1's STRICT mode (fsk_kernels.hip FS0-FS2 with
 * their step bounds, KF1-KF2): F2's margin for a split call becomes tau +
 * F ||ifft(h)||_1 / peak with F a bound on |z_split - z_serial| per tone that
 * holds for every input (the PSK strict mode's band-pass analysis per tone),
 * instead of tau + kappa ||ifft(h)||_1 (a measured premise).  Set: 1 on, 0
 * off, -1 the process default (AMR_FSK_SPLIT_STRICT=0 / 1).  split_strict:
 * whether this plan's split calls use it; last_strict: whether the last did. */
int amr_fsk_plan_set_split_strict(amr_fsk_plan *plan, int mode);
int amr_fsk_plan_split_strict(amr_fsk_plan *plan);
int amr_fsk_plan_last_strict(amr_fsk_plan *plan);
/* The strict band-pass design of ONE filter (host arithmetic; the tests'
 * restatement reads it): w the plan's warm-up (amr_fsk_split_design), consts
 * [32] in amr_psk_split_strict_design's layout (the low-pass fields 0), tabs
 * (NULL: not written) = kabs [w] | z0abs [w + 1] | W | K12 | HS | GS | TZ. */
int amr_fsk_split_strict_design(const double *b, const double *a, const double *zi, int ntaps, int64_t w,
                                double *consts, double *tabs);
/* Diagnostic (tests): the strict split F1 over a host batch: z_out
 * [n_streams][n_samples][2] (mark, space), bnd_out [n_streams][2][8] the
 * per-tone maxima as doubles (D1max, E1max, max|y1|, D2max, S1max, -, F, -),
 * peak_out [n_streams] max |ext x|.  Synchronous.  A plan without decision
 * bits is refused (AMR_E_INVALID), nothing written. */
int amr_fsk_split_bounds_host(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                              double *z_out, double *bnd_out, double *peak_out);
/* the split F1's band-pass output itself (a diagnostic the tests compare with
 * the oracle's restatement): out [n_streams][n_samples][2] (mark, space);
 * chunk 0 = the plan's rule (1..127 refused with the convolution starts on,
 * as amr_psk_split_symbols_host).  Synchronous. */
int amr_fsk_split_bandpass_host(amr_fsk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                                int64_t chunk, double *out);

/* ---- FFT / Hilbert (the transforms under scipy.signal.hilbert) --------------
 * in/out: [batch][n] interleaved complex doubles; inverse scales by 1/n
 * (numpy.fft.fft / numpy.fft.ifft).  analytic: [batch][n] complex doubles =
 * scipy.signal.hilbert(x) for real x [batch][n].  Synchronous, on `device`. */
int amr_fft_c2c_host(const double *in, double *out, int64_t n, int64_t batch, int inverse, int device);
int amr_hilbert_host(const double *x, double *analytic, int64_t n, int64_t batch, int device);
/* scipy.signal.resample(x, num) of each real row (x: [batch][nx] -> y: [batch][num]),
 * as decoder.decode_wav_file calls it (decoder.py:385-387), bit for bit:
 * pocketfft's rfft (every radix, Bluestein), the reference's spectrum
 * truncation / zero-padding with its Nyquist-bin rule, pocketfft's irfft,
 * times num/nx (pocketfft_dev.h). */
int amr_resample_host(const double *x, int64_t nx, int64_t num, int64_t batch, double *y, int device);
/* |scipy.signal.hilbert(x)| of each real row (x: [batch][n] -> env), evaluated
 * as pocketfft + numpy do, bit for bit (the FSK exact path's envelope stage,
 * modem.py:309; a diagnostic entry for tests) */
int amr_hilbert_env_exact_host(const double *x, int64_t n, int64_t batch, double *env, int device);

/* ---- FEC (fec.py:34-69) -----------------------------------------------------
 * in: [n][in_stride] bytes, in_len[n]; out: [n][out_stride] (>= in_len each);
 * crc_ok[s] = 1 when the recomputed CRC32 equals the trailing word
 * (the reference only prints "Aviso: CRC ..." on mismatch). */
int amr_fec_decode_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, int64_t n,
                        uint8_t *out, int64_t out_stride, int64_t *out_len, int32_t *crc_ok);

/* ---- FBP frame parse (decoder.py:142-208, parse_fbp_stream_enhanced) --------
 * For every stream's decoded bytes (in: [n][in_stride], in_len[n]): every
 * b'FBPC' occurrence in increasing order, run through the reference's checks
 * in its order, and the CRC32 (binascii.crc32) of the payload of those that
 * pass them.  n_cands[s] = occurrences found (may exceed max_cands: records
 * are kept for the first min(n_cands, max_cands, 256); a caller seeing more
 * parses that stream itself).  recs: [n][max_cands], 1 <= max_cands <=
 * AMR_FRAME_MAX_CANDS (larger is AMR_E_INVALID).  A header field that the
 * checks never reached (the ones read after the check that stopped the
 * candidate) is 0; calc_crc is set for OK / CRC_BAD.  The host turns records
 * into the reference's list of {'name', 'data', 'final_crc'} and log lines. */
#define AMR_FRAME_MAX_CANDS 256     /* records kept per stream (LDS list of k_frame_parse) */
#define AMR_FRAME_SHORT 0          /* start + 30 > len(raw)            decoder.py:165 */
#define AMR_FRAME_NONAME 1         /* name_len == 0                     decoder.py:169 */
#define AMR_FRAME_NOMETA 2         /* meta_start + 24 > len(raw)        decoder.py:177 */
#define AMR_FRAME_BADLEN 3         /* dlen > 50_000_000 or dlen == 0    decoder.py:182 */
#define AMR_FRAME_INCOMPLETE 4     /* payload past the end: "Dados incompletos"  :185-187 */
#define AMR_FRAME_CRC_BAD 5        /* "Erro de CRC"                     decoder.py:197-198 */
#define AMR_FRAME_OK 6             /* CRC valid: appended               decoder.py:190-196 */
#define AMR_FRAME_PENDING_CRC 7    /* internal */
typedef struct amr_frame_rec {
  int64_t start;                   /* index of the magic */
  int64_t name_start;              /* start + 5 */
  int64_t payload_start;           /* meta_start + 24 */
  int32_t status;                  /* AMR_FRAME_* */
  int32_t name_len;                /* raw[start + 4] */
  uint32_t part, total, fsize, fcrc, dlen, pcrc;   /* '<IIIIII' at meta_start */
  uint32_t calc_crc;               /* crc32(payload) when computed */
  uint32_t reserved;
} amr_frame_rec;                   /* 64 bytes */
int amr_frame_parse_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, int64_t n,
                         int64_t max_cands, int32_t *n_cands, amr_frame_rec *recs);
/* device pointers, enqueued on the plan's stream (plan may be NULL: the null stream) */
int amr_frame_parse_device(amr_psk_plan *plan, const uint8_t *d_in, int64_t in_stride, const int64_t *d_in_len,
                           int64_t n, int64_t max_cands, int32_t *d_n_cands, amr_frame_rec *d_recs);

/* ---- transmit side (modem.py:28-65, 138-186, 270-295, 360-368) ------------
 * The reference's modulators for a batch of payloads: data [n][data_stride]
 * bytes, n_bytes[n].  out [n][out_stride] float32: each stream's waveform
 * (bpsk_modulate / qpsk_modulate / fsk_modulate, sample for sample) cut or
 * zero-padded to n_out samples; pcm (optional, may be NULL) the same samples
 * as modem.wav_from_array writes them, int16(out * 32767).
 * f0 = carrier (PSK) or mark_freq (FSK); f1 = space_freq (FSK only).
 * A PSK symbol of 1..9 samples is the reference's numpy broadcast ValueError
 * (its 10 % ramp is empty, modem.py:58-61 / 181-183): AMR_E_INVALID with the
 * reference's message in amr_last_error(). */
#define AMR_TX_BPSK 0              /* bpsk_modulate  modem.py:28-65   */
#define AMR_TX_QPSK 1              /* qpsk_modulate  modem.py:138-186 */
#define AMR_TX_FSK 2               /* fsk_modulate   modem.py:270-295 */
/* hellschreiber_modulate (hellschreiber.py:109-152).  The payload is one glyph
 * index per character: 0..94 for ' '..'~', 255 for a character outside the
 * table (a blank 51-pixel cell); the caller decodes the text.  f0 = carrier.
 * baud / sample_rate rounding to 0 samples per pixel is the reference's
 * ValueError (np.max of an empty waveform; < 0: np.zeros of a negative size):
 * AMR_E_INVALID with numpy's message.  n_bytes counts characters. */
#define AMR_TX_HELL 3
/* d8psk_modulate (no reference counterpart): the bits
 * [0,0,0]*30 + [1,1,0]*10 + payload, zero-padded to a multiple of 3, taken
 * three at a time (MSB first) as a Gray-coded phase step of k * pi/4,
 * 40 + ceil(8 n_bytes / 3) symbols of sps = int(sample_rate / baud) samples:
 *   out[n] = float32(sin(((2 pi) f0) * (n / sample_rate) + phase[n / sps]) * env[n % sps])
 * -- the carrier runs in absolute time (phase-continuous), the envelope is the
 * PSK modulators' 10 % ramps, all ones when the ramp is empty (sps < 10 is
 * allowed); sps < 1 is AMR_E_INVALID. */
#define AMR_TX_D8PSK 4
/* star16_modulate (no reference counterpart): the bits
 * [0,0,0,0]*30 + [1,1,1,0]*10 + payload, four at a time (MSB first)
 * (a, b2, b1, b0): b2 b1 b0 steps the phase as d8psk's tribit does, a toggles
 * the ring (outer before the first symbol; A = 1.0 outer, 0.5 inner);
 * 40 + 2 n_bytes symbols of sps = int(sample_rate / baud) samples:
 *   out[n] = float32(sin(((2 pi) f0) * (n / sample_rate) + phase[n / sps]) * (env[n % sps] * A[n / sps]))
 *   env[i] = 4.0 * (u * (1.0 - u)),  u = (i + 0.5) / sps
 * -- the carrier in absolute time, a parabolic envelope at any sps >= 1;
 * sps < 1 is AMR_E_INVALID.  Its work buffer holds a phase and an amplitude
 * per symbol (amr_tx_work_bytes).  (Mode 5 is not assigned.) */
#define AMR_TX_STAR16 6
/* natural waveform length of an n_bytes payload (the reference's len(out)), or < 0 */
int64_t amr_tx_samples(int mode, int64_t n_bytes, double baud, double sample_rate);
/* device scratch bytes amr_modulate_device needs for this shape */
int64_t amr_tx_work_bytes(int mode, double baud, double sample_rate, int64_t n_streams, int64_t n_out);
int amr_modulate_host(int mode, double baud, double f0, double f1, double sample_rate, const uint8_t *data,
                      int64_t data_stride, const int64_t *n_bytes, int64_t n, float *out, int64_t out_stride,
                      int64_t n_out, int16_t *pcm, int64_t pcm_stride);
/* device pointers, enqueued on the plan's stream (plan may be NULL: the null stream) */
int amr_modulate_device(amr_psk_plan *plan, int mode, double baud, double f0, double f1, double sample_rate,
                        const uint8_t *d_data, int64_t data_stride, const int64_t *d_n_bytes, int64_t n,
                        float *d_out, int64_t out_stride, int64_t n_out, int16_t *d_pcm, int64_t pcm_stride,
                        void *d_work, int64_t work_bytes);

/* ---- Hellschreiber receiver (hellschreiber.py:155-187) ----------------------
 * x [n_streams][x_stride] elements of type `elem`, n_samples used per stream.
 * sps = int(round(sample_rate / baud)); pixel p of a stream is 1 iff
 * np.mean(x[p*sps:(p+1)*sps] ** 2) > 0.1, evaluated as numpy evaluates it for
 * that dtype (its pairwise summation order, squares in the array's dtype --
 * integers wrap --, float16 / float32 summed in float32, everything else in
 * float64, np.mean's result dtype and numpy's weak-scalar comparison); every
 * full group of 7 pixels gives one output byte (the first glyph with a row
 * equal to the 7-bit value, else '?').  out [n_streams][out_stride] bytes,
 * out_len[n_streams] = pixels / 7.  energy (optional, may be NULL):
 * [n_streams][pixels] float64, each pixel's np.mean value widened exactly.
 * sps == 0 is the reference's ValueError: AMR_E_INVALID with range()'s message
 * in amr_last_error(); a negative sps decodes nothing, as the reference. */
#define AMR_HELL_ELEM_F32 0
#define AMR_HELL_ELEM_F64 1
#define AMR_HELL_ELEM_F16 2
#define AMR_HELL_ELEM_I8 3         /* raw integers: their values (the square wraps in the dtype) */
#define AMR_HELL_ELEM_I16 4
#define AMR_HELL_ELEM_I32 5
#define AMR_HELL_ELEM_I64 6
#define AMR_HELL_ELEM_U8 7
#define AMR_HELL_ELEM_U16 8
#define AMR_HELL_ELEM_U32 9
#define AMR_HELL_ELEM_U64 10
#define AMR_HELL_ELEM_PCM16 11     /* int16 PCM read as int16 / 32768.0 in float64 (AMR_DTYPE_I16's meaning) */
/* pixels a capture of n_samples holds (n_samples / sps), or < 0 */
int64_t amr_hell_pixels(int64_t n_samples, double baud, double sample_rate);
/* device scratch bytes amr_hell_demod_device needs (the pixel's summation tree + the lookup) */
int64_t amr_hell_work_bytes(double baud, double sample_rate);
int amr_hell_demod_host(const void *x, int elem, int64_t n_streams, int64_t x_stride, int64_t n_samples, double baud,
                        double sample_rate, uint8_t *out, int64_t out_stride, int64_t *out_len, double *energy);
/* device pointers, enqueued on the plan's stream (plan may be NULL: the null stream) */
int amr_hell_demod_device(amr_psk_plan *plan, const void *d_x, int elem, int64_t n_streams, int64_t x_stride,
                          int64_t n_samples, double baud, double sample_rate, uint8_t *d_out, int64_t out_stride,
                          int64_t *d_out_len, double *d_energy, void *d_work, int64_t work_bytes);
/* the glyph bitmaps the library carries: rows [95][7] (' '..'~'; byte r = pixel
 * row r, bit i = its i-th pixel on the air) and the receiver's lookup [128];
 * either may be NULL.  Host only.  Returns the glyph count (95). */
int amr_hell_glyph_rows(uint8_t *rows, uint8_t *rx_lookup);

/* ---- convolutional code (fec.py:72-111) and its Viterbi decoder ---------------
 * Rate 1/2, K = 7, polynomials 171 / 133 octal, register ((sr << 1) | bit) & 0x7F,
 * message bits MSB-first then 6 zero flush bits, the coded bits packed MSB-first;
 * a message of n bytes is a codeword of 2 n + 2 bytes whose last byte holds the
 * final 4 bits in its LOW nibble (the reference's packing).  The encoder is
 * fec.ConvolutionalEncoder.encode for a batch.  The decoder is a
 * maximum-likelihood hard-decision Viterbi decoder over the whole codeword
 * (Hamming branch metrics, int32 path metrics, start and end in state 0, a tie
 * keeps the predecessor with the older bit clear); the reference has none -- its
 * ViterbiDecoder.decode is a stub.  A length L is a codeword length when it is
 * even and 2 <= L <= 2^24.  in [n][in_stride] bytes, in_len[n]; out
 * [n][out_stride] bytes, out_len[n]; metric[n] = the number of coded-bit
 * positions in which the input differs from the codeword of the decoded message
 * (the last byte's high nibble is not looked at).  Only out_len[i] bytes of an
 * output row are written. */
/* 2 n_bytes + 2, or < 0 for n_bytes < 0 */
int64_t amr_conv_encoded_len(int64_t n_bytes);
/* in_len[i] <= in_stride message bytes per row; out_stride >= 2 * longest + 2 */
int amr_conv_encode_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, int64_t n, uint8_t *out,
                         int64_t out_stride, int64_t *out_len);
/* device scratch bytes amr_viterbi_decode_device needs for n rows of in_stride bytes: 512 bytes of
 * survivor decisions per 64 trellis steps of the longest codeword a row can hold.  Host arithmetic. */
int64_t amr_viterbi_work_bytes(int64_t in_stride, int64_t n);
/* device pointers, enqueued on the plan's stream (plan may be NULL: the null stream).  The lengths are
 * read on the device: a row whose length is not a codeword length, or exceeds in_stride, gets
 * out_len 0 and metric -1 and nothing else of it is touched.  out_stride >= in_stride / 2 - 1. */
int amr_viterbi_decode_device(amr_psk_plan *plan, const uint8_t *d_in, int64_t in_stride, const int64_t *d_in_len,
                              int64_t n, uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int32_t *d_metric,
                              void *d_work, int64_t work_bytes);
/* host pointers; a length that is not a codeword length is AMR_E_INVALID (the message names the row)
 * before any device work; large batches are decoded in chunks of bounded scratch */
int amr_viterbi_decode_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, int64_t n, uint8_t *out,
                            int64_t out_stride, int64_t *out_len, int32_t *metric);

/* ---- soft decisions: PSK soft output and the soft-input Viterbi decoder ----
 * A soft value is an int8 v: v > 0 bit 1, v < 0 bit 0, |v| in 1..127 the reliability, 0 an erasure (the
 * demodulator never emits it; the decoder takes it -- punctured codes -- and reads -128 as -127).
 * For a differential product d = (dr, di) the sign is the bit the demodulator decides, the magnitude, in
 * fp64 in this order with den = |dr| + |di|:  QPSK hi bit r = |dr + di| / den, lo bit r = |dr - di| / den,
 * BPSK r = |dr| / den;  q = floor(r * 127.0 + 0.5);  1 unless q >= 1;  127 if q > 127;  else q.
 * soft[s][j], j < 8 * out_len[s], belongs to the j-th bit of the stream's output bytes: packing soft > 0
 * MSB-first gives out[s] again.  Only those values of a row are written.  The soft entries compute on the
 * reference's own symbol samples: they never run the time-split layout (a plan set to it runs the row
 * layout for the call), and they leave amr_psk_plan_last_layout() and its kin as the hard calls set them. */
/* amr_psk_demod_host's arguments, then edges (NULL, or as amr_psk_demod_host_edges), soft [B][soft_stride],
 * soft_stride >= 8 * amr_psk_plan_out_capacity() */
int amr_psk_demod_soft_host(amr_psk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                            uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx,
                            const double *edges, int8_t *soft, int64_t soft_stride);
/* the same with device pointers, asynchronous on the plan's stream */
int amr_psk_demod_soft_device(amr_psk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                              uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                              const double *d_edges, int8_t *d_soft, int64_t soft_stride);
/* the soft stage alone on given symbols (amr_psk_slice_host's counterpart): sym [n_streams][n_sym][re, im];
 * soft [n_streams][2 (n_sym - 1)] (QPSK) or [n_streams][n_sym - 1] (BPSK), every bit from 0, no sync */
int amr_psk_soft_host(int kind, const double *sym, int64_t n_streams, int64_t n_sym, int8_t *soft);
/* The soft-input decoder: amr_viterbi_decode_*'s code, trellis, tie rule and traceback with the branch
 * metric [c1 != (r1 > 0)] |r1| + [c2 != (r2 > 0)] |r2| for a step's values (r1, r2) and a branch's output
 * bits (c1, c2); metric[i] = the sum of |r| over the positions where the decoded message's codeword
 * disagrees with the input's sign.  With every |r| = 1 it is the hard decoder.  A row holds n_vals values
 * after the in_offset leading ones every row skips (so it can follow a soft demodulation without a copy):
 * n_vals % 16 == 12, the coded bit stream (two values per step), or n_vals % 16 == 0 (>= 16), the
 * byte-aligned image of a codeword of n_vals / 8 bytes whose last byte's high nibble (four values) is
 * skipped; at most 2^21 - 4 values. */
/* device scratch bytes for n rows of in_stride_vals values: 512 bytes per 64 steps of the longest row */
int64_t amr_viterbi_soft_work_bytes(int64_t in_stride_vals, int64_t n);
/* device pointers, on the plan's stream (plan may be NULL).  A row whose length is none of the above, or
 * exceeds in_stride - in_offset, gets out_len 0 and metric -1 and nothing else of it is touched. */
int amr_viterbi_decode_soft_device(amr_psk_plan *plan, const int8_t *d_in, int64_t in_stride, int64_t in_offset,
                                   const int64_t *d_in_len, int64_t n, uint8_t *d_out, int64_t out_stride,
                                   int64_t *d_out_len, int32_t *d_metric, void *d_work, int64_t work_bytes);
/* host pointers; a bad length is AMR_E_INVALID (the message names the row) before any device work */
int amr_viterbi_decode_soft_host(const int8_t *in, int64_t in_stride, int64_t in_offset, const int64_t *in_len,
                                 int64_t n, uint8_t *out, int64_t out_stride, int64_t *out_len, int32_t *metric);

/* ---- Reed-Solomon over GF(2^8) (fec.ReedSolomonCodec) -----------
 * No reference counterpart: the reference's "Reed-Solomon" is the parity stub amr_fec_decode_host
 * reproduces.  Field polynomial 0x11D, alpha = 2, generator prod_{i < nsym} (x - alpha^i), 2 <= nsym <= 64,
 * k = 255 - nsym.  Systematic: a message of n bytes is ceil(n / k) blocks of k bytes (the last 1 .. k), each
 * followed by its nsym parity bytes -- the remainder of m(x) x^nsym by g, the block's first byte the highest
 * power; short blocks are shortened codewords.  A received length L is valid when L == 0 or the last block,
 * L - 255 (ceil(L / 255) - 1) bytes, holds at least nsym + 1.  interleave (1 .. 64; 1: none): consecutive
 * blocks form groups of `interleave` (the last group may have fewer), and a group's bytes are sent column
 * by column -- byte c of every block of the group that has a byte c, for c = 0, 1, ...
 * Decoding: a block with f erased positions decodes to the codeword that differs from it in e positions
 * outside the erased set with 2 e + f <= nsym (it is unique; received values at erased positions are
 * ignored); where there is none the block FAILS and its message bytes pass through as received.
 * corrected[i] = the byte positions of row i's decoded blocks where the codeword differs from the received
 * block, failed[i] = its failed blocks.  Only out_len[i] bytes of an output row are written. */
/* n + ceil(n / (255 - nsym)) nsym, or < 0 for a bad argument */
int64_t amr_rs_encoded_len(int64_t n, int nsym);
/* the message bytes of a received length L, or -1 when L is not valid (or nsym is out of range) */
int64_t amr_rs_decoded_len(int64_t L, int nsym);
/* device pointers, enqueued on the plan's stream (plan may be NULL: the null stream).  The lengths are read
 * on the device: a row whose length is outside [0, in_stride] gets out_len -1 and nothing else of it is
 * touched.  out_stride >= amr_rs_encoded_len(in_stride, nsym). */
int amr_rs_encode_device(amr_psk_plan *plan, const uint8_t *d_in, int64_t in_stride, const int64_t *d_in_len,
                         int64_t n, int nsym, int interleave, uint8_t *d_out, int64_t out_stride,
                         int64_t *d_out_len);
/* host pointers; a length outside [0, in_stride] is AMR_E_INVALID (the message names the row) */
int amr_rs_encode_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, int64_t n, int nsym,
                       int interleave, uint8_t *out, int64_t out_stride, int64_t *out_len);
/* device pointers, on the plan's stream (plan may be NULL).  d_erase is NULL or [n][in_stride] bytes in the
 * layout of d_in, nonzero = erased.  A row whose length is not valid, or exceeds in_stride, gets out_len 0,
 * corrected 0 and failed -1 and nothing else of it is touched.  out_stride >= the message bytes of the
 * longest valid length <= in_stride. */
int amr_rs_decode_device(amr_psk_plan *plan, const uint8_t *d_in, int64_t in_stride, const int64_t *d_in_len,
                         const uint8_t *d_erase, int64_t n, int nsym, int interleave, uint8_t *d_out,
                         int64_t out_stride, int64_t *d_out_len, int32_t *d_corrected, int32_t *d_failed);
/* host pointers; a length that is not valid is AMR_E_INVALID (the message names the row) before any device work */
int amr_rs_decode_host(const uint8_t *in, int64_t in_stride, const int64_t *in_len, const uint8_t *erase, int64_t n,
                       int nsym, int interleave, uint8_t *out, int64_t out_stride, int64_t *out_len,
                       int32_t *corrected, int32_t *failed);

/* ---- ofdm: a multi-carrier DQPSK modem (no reference counterpart: the
 * reference's ofdm_*_simple ignore num_subcarriers and call QPSK; DESIGN.md
 * §3j, tests/ofdm_cases.py) ---------------------------------------------------
 * Geometry for (sps, K): one OFDM symbol is L = K * sps samples, the cyclic
 * prefix Ncp = L / 8 of them, Nu = L - Ncp the useful part; subcarrier k sits
 * on DFT bin bins[k] = bins[0] + k of the Nu useful samples.  Valid iff
 * 1 <= K <= 64, sps >= 1, bins[0] >= 1 and 2 * bins[K-1] < Nu; anything else
 * is AMR_E_INVALID before any device work.
 * W: the caller's twiddle table [K][Nu][2] float64, (cos th, -sin th) with
 * th = (2 pi) * (((bins[k] * m) % Nu) / Nu).
 * Receiver: S = n_samples / L symbols per stream (a partial tail is ignored),
 *   Y[s][k] = sum_m x[s*L + Ncp + m] * W[k][m]      in four interleaved partial
 * sums p[m & 3], each sequential in m from 0.0, every product rounded before
 * it is added (no fma), combined as (p0 + p1) + (p2 + p3) per component;
 * d = Y[s+1][k] * conj(Y[s][k]) (numpy's multiply, as the PSK slicers), and
 * with ar = |dr|, ai = |di|:  ai < ar: m = dr > 0 ? 0 : 2;  else m = di > 0 ?
 * 1 : 3;  the dibit is {0, 1, 3, 2}[m], MSB first, in the order j = s*K + k:
 * 2 K (S - 1) bits per stream in one string; sync search and byte pack as for
 * the PSK plans.  S < 2: no bytes, sync index -1.
 * Soft values: two int8 per product, the hard bit's sign, the magnitudes of
 * amr_psk_soft_host's QPSK rule, aligned to the bytes as amr_psk_demod_soft_*. */
typedef struct amr_ofdm_plan amr_ofdm_plan;
#define AMR_TO_DFT 0          /* k_ofdm_dft */
#define AMR_TO_SLICE 1        /* k_ofdm_slice */
#define AMR_TO_SYNC_PACK 2    /* sync search and byte pack; in a soft call k_ofdm_soft too (it reads their window) */
#define AMR_TO_LAUNCH 3       /* the whole launch */
#define AMR_TO_ACQUIRE 4      /* k_ofdm_fold and k_ofdm_acq_min of an acquiring call (inside AMR_TO_LAUNCH) */
#define AMR_TO_COUNT 5
int amr_ofdm_plan_create(amr_ofdm_plan **plan, int device, int64_t n_samples, int64_t sps, int K,
                         const int32_t *bins, const double *W, int64_t max_streams);
int amr_ofdm_plan_destroy(amr_ofdm_plan *plan);
int amr_ofdm_plan_synchronize(amr_ofdm_plan *plan);
int amr_ofdm_plan_enable_timing(amr_ofdm_plan *plan, int on);
/* milliseconds of each AMR_TO_* slot in the last call (-1 = not run) */
int amr_ofdm_plan_timings(amr_ofdm_plan *plan, float *ms, int count);
/* bytes an output row needs (2 K (S - 1) / 8 + 1), or -1 */
int64_t amr_ofdm_plan_out_capacity(const amr_ofdm_plan *plan);
/* device bytes the plan holds now, and (host arithmetic) what a plan of this
 * shape holds once its host entries have staged a full batch; < 0: bad shape */
int64_t amr_ofdm_plan_scratch_bytes(const amr_ofdm_plan *plan);
int64_t amr_ofdm_plan_bytes_estimate(int64_t n_samples, int64_t sps, int K, int64_t max_streams);
/* the PSK entries' shapes: x [n_streams][x_stride] samples of `dtype`, out
 * [n_streams][out_stride] bytes (out_stride >= out_capacity - 1), lengths and
 * sync indices; soft [n_streams][soft_stride], soft_stride >= 8 * out_capacity */
int amr_ofdm_demod_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                        uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx);
int amr_ofdm_demod_device(amr_ofdm_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                          uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx);
int amr_ofdm_demod_soft_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx, int8_t *soft,
                             int64_t soft_stride);
int amr_ofdm_demod_soft_device(amr_ofdm_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                               uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                               int8_t *d_soft, int64_t soft_stride);
/* the DFT stage alone: Y [n_streams][S][K][2] float64 (re, im) */
int amr_ofdm_symbols_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                          double *Y);
/* ---- ofdm acquisition: the symbol boundary of an unaligned capture (DESIGN.md
 * §3k, tests/ofdm_acquire_cases.py).  Float64, no fma, samples read as the
 * receiver reads them; per stream of n samples, with Q = 64:
 *   M = (n - Nu) / L if n >= Nu + L, else 0
 *   g_q[r] = sum over s = 64 q .. min(64 q + 64, M) - 1 of d * d,
 *            d = x[s L + r] - x[s L + r + Nu],   sequential in s from 0.0
 *   G[r]  = g_0[r] + g_1[r] + ...                sequential in q from 0.0
 *   E[d]  = sum over i = 0 .. Ncp - 1 of G[(d + i) % L], sequential in i from 0.0
 *   dhat  = best after: best = 0; for d = 1 .. L - 1: if (E[d] < E[best]) best = d
 *   o     = dhat - Ncp / 2;  if (o > L - 1 - Ncp) o -= L      in [-Ncp, L - 1 - Ncp]
 * The acquired demodulation of x is the demodulation above of shift(x, o):
 * shift(x, o)[i] = x[i + o] where 0 <= i + o < n, else 0.0, the length n kept;
 * S, the bit count, the output capacity and the sync search are unchanged.
 * L < 8 has no prefix (Ncp = 0): E is zeros, o = 0, nothing is acquired.
 * The work buffers are allocated on the plan's first acquiring call (then part
 * of amr_ofdm_plan_scratch_bytes); amr_ofdm_acquire_bytes_estimate is their
 * size by host arithmetic (< 0: bad shape). */
int64_t amr_ofdm_acquire_bytes_estimate(int64_t n_samples, int64_t sps, int K, int64_t max_streams);
/* the acquisition stage alone: offset [n_streams] (o), dhat [n_streams] and E
 * [n_streams][L]; dhat and E may be NULL.  _device: device pointers, queued on
 * the plan's stream. */
int amr_ofdm_acquire_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                          int64_t *offset, int64_t *dhat, double *E);
int amr_ofdm_acquire_device(amr_ofdm_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                            int64_t *d_offset, int64_t *d_dhat, double *d_E);
/* the DFT stage at given offsets: Y of shift(x[b], offset[b]); an offset outside
 * [-Ncp, L - 1 - Ncp] is AMR_E_INVALID before any device work */
int amr_ofdm_symbols_at_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             const int64_t *offset, double *Y);
/* amr_ofdm_demod_soft_* with the acquisition in front, all on the plan's stream
 * with no host round trip in between; the offsets to offset [n_streams].  soft
 * and offset may be NULL (soft_stride is then ignored). */
int amr_ofdm_demod_acq_host(amr_ofdm_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                            uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx, int8_t *soft,
                            int64_t soft_stride, int64_t *offset);
int amr_ofdm_demod_acq_device(amr_ofdm_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                              uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                              int8_t *d_soft, int64_t soft_stride, int64_t *d_offset);
/* the slicer and soft stages alone on given Y [n_streams][n_sym][K][2]: words
 * [n_streams][max(1, ceil(2 K (n_sym - 1) / 32))] (MSB first), soft
 * [n_streams][2 K (n_sym - 1)] (every bit from 0) */
int amr_ofdm_slice_host(const double *Y, int64_t n_streams, int64_t n_sym, int K, uint32_t *words);
int amr_ofdm_soft_host(const double *Y, int64_t n_streams, int64_t n_sym, int K, int8_t *soft);
/* ofdm_modulate: the bits [0,0]*30 + [1,1]*10 + payload, zero-padded to a
 * multiple of 2 K; dibit j on symbol 1 + j / K, subcarrier j % K, as a phase
 * step 00 -> 0, 01 -> pi/2, 11 -> pi, 10 -> -pi/2 added sequentially to symbol
 * 0's Newman phases (pi * (k*k)) / K.  The geometry from sps = int(sample_rate
 * / baud) and c0 = floor(carrier * Nu / sample_rate + 0.5), bins[k] = c0 - K/2
 * + k.  Sample i of symbol s, m = (i - Ncp) mod Nu:
 *   float32((sum_k sin((2 pi) * (((bins[k]*m) % Nu) / Nu) + ph[s][k])) * (1.0 / K))
 * the sum sequential in k from 0.0.  out / pcm / n_out as amr_modulate_host. */
int amr_ofdm_modulate_host(double baud, double carrier, double sample_rate, int K, const uint8_t *data,
                           int64_t data_stride, const int64_t *n_bytes, int64_t n, float *out, int64_t out_stride,
                           int64_t n_out, int16_t *pcm, int64_t pcm_stride);

/* ---- spread: a direct-sequence DBPSK modem with code acquisition (no
 * reference counterpart: the reference's dsss_modulate calls BPSK and it has
 * no dsss_demodulate; DESIGN.md §3l, tests/spread_cases.py) ---------------------
 * Geometry for (spc, C, cyc): spc samples per chip, C chips per bit, one bit is
 * L = C * spc samples and holds cyc whole carrier cycles.  Valid iff
 * 2 <= C <= 64, spc >= 1, cyc >= 1, 2 * cyc < L and L <= 2^24; anything else is
 * AMR_E_INVALID before any device work.
 * Tables (the caller's, float64), over i = 0 .. L-1 with th = (2 pi) *
 * (((cyc * i) % L) / L) and sg[i] = cs[i / spc]:  Wc [L][2] = (cos th, -sin th),
 * T [L][2] = sg[i] * Wc[i], Sn [L] = sin th; cs [C] the chip signs, +1.0 for a
 * code bit 0 and -1.0 for a 1.
 * Receiver at offset o in [0, L-1] (0 when not acquired): x' = shift(x, o),
 * shift(x, o)[i] = x[i + o] while i + o < n, else 0.0; S = n_samples / L,
 *   Y[s] = sum_i x'[s*L + i] * T[i]        in four interleaved partial sums
 * p[i & 3], each sequential in i from 0.0, every product rounded before it is
 * added (no fma), combined as (p0 + p1) + (p2 + p3) per component;
 * d = Y[s+1] * conj(Y[s]) (numpy's multiply, as the PSK slicers); the bit is
 * 1 iff dr < 0 (NaN and zeros give 0): S - 1 bits per stream, sync search and
 * byte pack as for the PSK plans.  S < 2: no bytes, sync index -1.
 * Soft values: one int8 per product, the hard bit's sign, the magnitude of
 * amr_psk_soft_host's BPSK rule, aligned to the bytes as amr_psk_demod_soft_*.
 * Acquisition, per stream of n samples:
 *   u[m]  = sum over i < spc of x[m + i] * Wc[(m + i) % L],  m = 0 .. n - spc,
 *           sequential in i from 0.0, the product rounded first
 *   M     = (n - L + 1) / L if n >= 2 L - 1, else 0
 *   y     = sum over j < C of cs[j] * u[d + s L + j spc], sequential in j from 0.0
 *   g_q[d] = sum over s = 64 q .. min(64 q + 64, M) - 1 of yr*yr + yi*yi, sequential from 0.0
 *   P[d]  = g_0[d] + g_1[d] + ...          sequential in q from 0.0
 *   o     = best after: best = 0; for d = 1 .. L - 1: if (P[d] > P[best]) best = d
 * The acquisition buffers are allocated on the plan's first acquiring call
 * (then part of amr_dsss_plan_scratch_bytes); amr_dsss_acquire_bytes_estimate is
 * their size by host arithmetic (< 0: bad shape).  n_samples < 2^31 to acquire. */
typedef struct amr_dsss_plan amr_dsss_plan;
#define AMR_TD_DESPREAD 0     /* k_dsss_despread */
#define AMR_TD_SLICE 1        /* k_dsss_slice */
#define AMR_TD_SYNC_PACK 2    /* sync search and byte pack; in a soft call k_dsss_soft too (it reads their window) */
#define AMR_TD_LAUNCH 3       /* the whole launch */
#define AMR_TD_ACQUIRE 4      /* k_dsss_acquire and k_dsss_acq_max of an acquiring call (inside AMR_TD_LAUNCH) */
#define AMR_TD_COUNT 5
int amr_dsss_plan_create(amr_dsss_plan **plan, int device, int64_t n_samples, int64_t spc, int C, int64_t cyc,
                         const double *Wc, const double *T, const double *cs, int64_t max_streams);
int amr_dsss_plan_destroy(amr_dsss_plan *plan);
int amr_dsss_plan_synchronize(amr_dsss_plan *plan);
int amr_dsss_plan_enable_timing(amr_dsss_plan *plan, int on);
/* milliseconds of each AMR_TD_* slot in the last call (-1 = not run) */
int amr_dsss_plan_timings(amr_dsss_plan *plan, float *ms, int count);
/* bytes an output row needs ((S - 1) / 8 + 1), or -1 */
int64_t amr_dsss_plan_out_capacity(const amr_dsss_plan *plan);
/* device bytes the plan holds now, and (host arithmetic) what a plan of this
 * shape holds once its host entries have staged a full batch; < 0: bad shape */
int64_t amr_dsss_plan_scratch_bytes(const amr_dsss_plan *plan);
int64_t amr_dsss_plan_bytes_estimate(int64_t n_samples, int64_t spc, int C, int64_t max_streams);
int64_t amr_dsss_acquire_bytes_estimate(int64_t n_samples, int64_t spc, int C, int64_t max_streams);
/* the PSK entries' shapes and argument contract.  soft [n_streams][soft_stride]
 * (soft_stride >= 8 * out_capacity) and offset [n_streams] may be NULL; acquire
 * != 0: every stream is read from its acquired offset, else from 0 (offset then
 * receives zeros).  Acquisition, despreader, slicer, sync / pack and soft values
 * are queued on the plan's stream with no host round trip in between. */
int amr_dsss_demod_host(amr_dsss_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                        uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx, int8_t *soft,
                        int64_t soft_stride, int64_t *offset, int acquire);
int amr_dsss_demod_device(amr_dsss_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                          uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                          int8_t *d_soft, int64_t soft_stride, int64_t *d_offset, int acquire);
/* the acquisition stage alone: offset [n_streams] and P [n_streams][L]; P may
 * be NULL.  _device: device pointers, queued on the plan's stream. */
int amr_dsss_acquire_host(amr_dsss_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                          int64_t *offset, double *P);
int amr_dsss_acquire_device(amr_dsss_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                            int64_t *d_offset, double *d_P);
/* the despreader alone at given offsets: Y [n_streams][S][2] of shift(x[b],
 * offset[b]); an offset outside [0, L - 1] is AMR_E_INVALID before any device work */
int amr_dsss_symbols_at_host(amr_dsss_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                             const int64_t *offset, double *Y);
/* the slicer and soft stages alone on given Y [n_streams][n_sym][2]: words
 * [n_streams][max(1, ceil((n_sym - 1) / 32))] (MSB first), soft
 * [n_streams][n_sym - 1] (every bit from 0) */
int amr_dsss_slice_host(const double *Y, int64_t n_streams, int64_t n_sym, uint32_t *words);
int amr_dsss_soft_host(const double *Y, int64_t n_streams, int64_t n_sym, int8_t *soft);
/* spread_modulate: the bits [1,0]*40 + payload (MSB first) as symbols s[0] =
 * +1.0, s[k+1] = -s[k] if bit k is 1 else s[k]; sample i of symbol k is
 * float32(s[k] * (sg[i] * Sn[i])): the sine is the caller's table, so the
 * output is the restatement's bit for bit.  No envelope ramp.  A frame of an
 * n_bytes payload is (81 + 8 n_bytes) * L samples; out / pcm / n_out as
 * amr_modulate_host. */
int amr_dsss_modulate_host(int64_t spc, int C, int64_t cyc, const double *cs, const double *Sn, const uint8_t *data,
                           int64_t data_stride, const int64_t *n_bytes, int64_t n, float *out, int64_t out_stride,
                           int64_t n_out, int16_t *pcm, int64_t pcm_stride);

/* ---- minshift: an MSK modem with bit-timing recovery (no reference
 * counterpart: the reference's msk_modulate calls FSK with tone spacing baud
 * and it has no msk_demodulate; DESIGN.md §3m, tests/minshift_cases.py) --------
 * Geometry for (L, cyc4): L samples per bit, h = L / 2, cyc4 quarter-cycles of
 * carrier per bit; a 1 bit advances the phase by cyc4 + 1 quarter-cycles, a 0
 * bit by cyc4 - 1.  Valid iff L >= 4, cyc4 >= 2, cyc4 + 1 < 2 L and L <= 2^24;
 * anything else is AMR_E_INVALID before any device work.
 * Tables (the caller's, float64): Sn [4 L] = sin((2 pi) * (p / (4 L)));
 * U [L][2] = (cos th, -sin th), th = (2 pi) * (((cyc4 * i) % (4 L)) / (4 L));
 * E0, E1 [2 L][2] = (cos th, -sin th), th = (2 pi) * ((((cyc4 -/+ 1) * r) %
 * (2 L)) / (2 L)); R [L][2] = (cos, +sin)((2 pi) * (d / L)).
 * Receiver at offset o in [0, L-1] (0 when not acquired): x' = shift(x, o) as
 * for spread; Sw = max(0, (n + h) / L - 1) windows,
 *   W[k] = sum over i < L of x'[(k+1) L - h + i] * U[i]
 * in four interleaved partial sums p[i & 3], each sequential in i from 0.0,
 * every product rounded before it is added (no fma), combined as (p0 + p1) +
 * (p2 + p3) per component; D[k] = (W[k+1] * conj(W[k])) * (-i)^(cyc4 mod 4)
 * (numpy's multiply, as the PSK slicers; the quarter-turns a swap and
 * negation); the bit is 1 iff D.imag > 0 (NaN and zeros give 0): Sw - 1 bits
 * per stream, sync search and byte pack as for the PSK plans.  Sw < 2: no
 * bytes, sync index -1.
 * Soft values: one int8 per product, the hard bit's sign, the magnitude of
 * amr_psk_soft_host's BPSK rule with D.imag in the role of the real part,
 * aligned to the bytes as amr_psk_demod_soft_*.
 * Bit timing, per stream of n samples, t = 0, 1:
 *   c_t   = sum over m < n of (x[m] * x[m]) * E_t[m % (2 L)], the square rounded
 *           first, then each component product.  Order: segments of 4096
 *           samples; in a segment partial j of 64 adds m = 4096 seg + 64 a + j
 *           sequentially in a from 0.0; the partials by the tree j with j + 32,
 *           then 16, 8, 4, 2, 1; the segment sums in order from 0.0
 *   q     = c1 * conj(c0) = (c1r c0r + c1i c0i, c1i c0r - c1r c0i)
 *   P[d]  = q.re * R[d].re - q.im * R[d].im
 *   o     = best after: best = 0; for d = 1 .. L - 1: if (P[d] > P[best]) best = d
 * The bit-timing buffers are allocated on the plan's first acquiring call
 * (then part of amr_msk_plan_scratch_bytes); amr_msk_acquire_bytes_estimate is
 * their size by host arithmetic (< 0: bad shape).  The timing slots are
 * AMR_TD_*: AMR_TD_DESPREAD is k_msk_corr, AMR_TD_ACQUIRE k_msk_lines and
 * k_msk_acq_max. */
typedef struct amr_msk_plan amr_msk_plan;
int amr_msk_plan_create(amr_msk_plan **plan, int device, int64_t n_samples, int64_t L, int64_t cyc4, const double *U,
                        const double *E0, const double *E1, const double *R, int64_t max_streams);
int amr_msk_plan_destroy(amr_msk_plan *plan);
int amr_msk_plan_synchronize(amr_msk_plan *plan);
int amr_msk_plan_enable_timing(amr_msk_plan *plan, int on);
/* milliseconds of each AMR_TD_* slot in the last call (-1 = not run) */
int amr_msk_plan_timings(amr_msk_plan *plan, float *ms, int count);
/* bytes an output row needs ((Sw - 1) / 8 + 1), or -1 */
int64_t amr_msk_plan_out_capacity(const amr_msk_plan *plan);
/* device bytes the plan holds now, and (host arithmetic) what a plan of this
 * shape holds once its host entries have staged a full batch; < 0: bad shape */
int64_t amr_msk_plan_scratch_bytes(const amr_msk_plan *plan);
int64_t amr_msk_plan_bytes_estimate(int64_t n_samples, int64_t L, int64_t max_streams);
int64_t amr_msk_acquire_bytes_estimate(int64_t n_samples, int64_t L, int64_t max_streams);
/* the amr_dsss_demod_* shapes and argument contract: soft and offset may be
 * NULL; acquire != 0: every stream is read from its acquired offset, else from
 * 0 (offset then receives zeros).  Bit timing, correlator, slicer, sync / pack
 * and soft values are queued on the plan's stream with no host round trip in
 * between. */
int amr_msk_demod_host(amr_msk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                       uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx, int8_t *soft,
                       int64_t soft_stride, int64_t *offset, int acquire);
int amr_msk_demod_device(amr_msk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                         int8_t *d_soft, int64_t soft_stride, int64_t *d_offset, int acquire);
/* the bit-timing stage alone: offset [n_streams] and q [n_streams][2]; q may
 * be NULL.  _device: device pointers, queued on the plan's stream. */
int amr_msk_acquire_host(amr_msk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                         int64_t *offset, double *q);
int amr_msk_acquire_device(amr_msk_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                           int64_t *d_offset, double *d_q);
/* the correlator alone at given offsets: W [n_streams][Sw][2] of shift(x[b],
 * offset[b]); an offset outside [0, L - 1] is AMR_E_INVALID before any device work */
int amr_msk_symbols_at_host(amr_msk_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                            const int64_t *offset, double *W);
/* the score and maximum stage alone on given line sums c [n_streams][4] =
 * (c0.re, c0.im, c1.re, c1.im), taken as one segment (0.0 + c); R [L][2];
 * offset [n_streams], q [n_streams][2] or NULL */
int amr_msk_offset_host(int64_t L, const double *R, const double *c, int64_t n_streams, int64_t *offset, double *q);
/* the slicer and soft stages alone on given W [n_streams][n_win][2]: words
 * [n_streams][max(1, ceil((n_win - 1) / 32))] (MSB first), soft
 * [n_streams][n_win - 1] (every bit from 0); cyc4 >= 0, only cyc4 mod 4 counts */
int amr_msk_slice_host(const double *W, int64_t n_streams, int64_t n_win, int64_t cyc4, uint32_t *words);
int amr_msk_soft_host(const double *W, int64_t n_streams, int64_t n_win, int64_t cyc4, int8_t *soft);
/* minshift_modulate: the bits [0] + [1,0]*40 + payload (MSB first) + [0]; the
 * integer phase p in units of 1 / (4 L) cycle, p_0 = 0, p_{k+1} = (p_k + L *
 * inc_k) % (4 L), inc_k = cyc4 + 1 for a 1 and cyc4 - 1 for a 0; sample i of bit
 * k is float32(Sn[(p_k + i * inc_k) % (4 L)]): the sine is the caller's table,
 * so the output is the restatement's bit for bit.  A frame of an n_bytes
 * payload is (82 + 8 n_bytes) * L samples; out / pcm / n_out as
 * amr_modulate_host. */
int amr_msk_modulate_host(int64_t L, int64_t cyc4, const double *Sn, const uint8_t *data, int64_t data_stride,
                          const int64_t *n_bytes, int64_t n, float *out, int64_t out_stride, int64_t n_out,
                          int16_t *pcm, int64_t pcm_stride);

/* ---- tone8: an 8-FSK modem with Costas sync (no reference counterpart: the
 * reference's ft8_modulate calls FSK with two tones at 50 Bd; DESIGN.md §3n,
 * tests/tone8_cases.py) ------------------------------------------------------
 * Geometry for (L, c2, search): L samples per symbol, T = L / 8 samples per
 * time slot, c2 half-cycles of carrier per symbol; tone m (0..7) has c2 + 2 m.
 * G = search half tone spacings are looked through either way: the lines f =
 * c2 - G .. c2 + 14 + G, NB = 15 + 2 G of them.  Valid iff L % 8 == 0, L <=
 * 2^24, 0 <= G <= 16, c2 - G >= 2 and c2 + 14 + G < L; anything else is
 * AMR_E_INVALID before any device work.  E [2 L][2] = (cos th, -sin th), th =
 * (2 pi) * (r / (2 L)), is the caller's table (numpy's libm).  A frame is the
 * Costas block 3, 1, 4, 0, 6, 5, 2, then the payload's tribits (MSB first,
 * zero-padded), tribit v on tone v ^ (v >> 1); nothing is differential.
 * Acquisition, float64, no fma, every product rounded before it is added:
 *   Z[j][f]  = sum_{i<T} x[j T + i] * E[(f (j T + i)) % (2 L)], sequential in i from 0.0, j < J = n / T
 *   Wd[j][f] = ((Z[j] + Z[j+1]) + (Z[j+2] + Z[j+3])) + ((Z[j+4] + Z[j+5]) + (Z[j+6] + Z[j+7])), j < J - 7
 *   P[j][f]  = re * re + im * im
 *   S[j][g]  = sum over s = 0..6 in order from 0.0 of P[j + 8 s][c2 + g + 2 costas[s]], j < nj = J - 55, |g| <= G
 *   (j*, g*) = best after: best = (0, -G); for j ascending, g ascending: if (S[j][g] > S[best]) best = (j, g)
 *   start = j* T, shift = g*, score = S[j*][g*]; nj <= 0: start = 0, shift = 0, score = 0.0
 * Demodulation reads stream b from o = start % L with every tone moved by
 * shift half-cycles per symbol (samples past the capture 0.0):
 *   Y[k][m]  = sum_{i<L} x[o + k L + i] * E[((c2 + g + 2 m) i) % (2 L)], k < S = n / L: four interleaved
 *              partial sums p[i & 3], each sequential in i from 0.0, (p0 + p1) + (p2 + p3)
 *   tone     = the first maximum of e_m = re * re + im * im from m = 0 (strictly greater; a NaN never wins)
 *   bits     = the tone's tribit t ^ (t >> 1) ^ (t >> 2), MSB first: 3 S bits into the PSK sync search and pack
 *   soft     = one int8 per bit: a1 / a0 the largest e_m among the four tones whose tribit has the bit set /
 *              clear (a NaN loses), magnitude as amr_psk_demod_soft_* from |a1 - a0| over a1 + a0, the hard bit's sign
 * The acquisition buffers are allocated on the plan's first acquiring call
 * (then part of amr_tone8_plan_scratch_bytes); amr_tone8_acquire_bytes_estimate
 * is their size by host arithmetic (< 0: bad shape).  The timing slots are
 * AMR_TD_*: AMR_TD_DESPREAD is k_tone8_dft, AMR_TD_ACQUIRE k_tone8_acq and
 * k_tone8_acq_max. */
typedef struct amr_tone8_plan amr_tone8_plan;
/* start slots one acquisition workgroup takes at this search (the kernel's chunk C), or < 0 */
int64_t amr_tone8_chunk(int64_t search);
int amr_tone8_plan_create(amr_tone8_plan **plan, int device, int64_t n_samples, int64_t L, int64_t c2, int64_t search,
                          const double *E, int64_t max_streams);
int amr_tone8_plan_destroy(amr_tone8_plan *plan);
int amr_tone8_plan_synchronize(amr_tone8_plan *plan);
int amr_tone8_plan_enable_timing(amr_tone8_plan *plan, int on);
/* milliseconds of each AMR_TD_* slot in the last call (-1 = not run) */
int amr_tone8_plan_timings(amr_tone8_plan *plan, float *ms, int count);
/* bytes an output row needs (3 S / 8 + 1), or -1 */
int64_t amr_tone8_plan_out_capacity(const amr_tone8_plan *plan);
/* device bytes the plan holds now, and (host arithmetic) what a plan of this
 * shape holds once its host entries have staged a full batch; < 0: bad shape */
int64_t amr_tone8_plan_scratch_bytes(const amr_tone8_plan *plan);
int64_t amr_tone8_plan_bytes_estimate(int64_t n_samples, int64_t L, int64_t search, int64_t max_streams);
int64_t amr_tone8_acquire_bytes_estimate(int64_t n_samples, int64_t L, int64_t search, int64_t max_streams);
/* the amr_msk_demod_* shapes and argument contract: soft, start and shift may
 * be NULL; acquire != 0: every stream is read at its acquired (start, shift),
 * else at (0, 0) (start and shift then receive zeros).  Acquisition, DFT,
 * slicer, sync / pack and soft values are queued on the plan's stream with no
 * host round trip in between. */
int amr_tone8_demod_host(amr_tone8_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t *out, int64_t out_stride, int64_t *out_len, int64_t *sync_idx, int8_t *soft,
                         int64_t soft_stride, int64_t *start, int64_t *shift, int acquire);
int amr_tone8_demod_device(amr_tone8_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                           uint8_t *d_out, int64_t out_stride, int64_t *d_out_len, int64_t *d_sync_idx,
                           int8_t *d_soft, int64_t soft_stride, int64_t *d_start, int64_t *d_shift, int acquire);
/* the acquisition stage alone: start, shift [n_streams] and score [n_streams];
 * score may be NULL.  _device: device pointers, queued on the plan's stream. */
int amr_tone8_acquire_host(amr_tone8_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                           int64_t *start, int64_t *shift, double *score);
int amr_tone8_acquire_device(amr_tone8_plan *plan, const void *d_x, int dtype, int64_t n_streams, int64_t x_stride,
                             int64_t *d_start, int64_t *d_shift, double *d_score);
/* the DFT alone at given per-stream (offset, shift): Y [n_streams][S][8][2];
 * an offset outside [0, L - 1] or a shift outside [-search, search] is
 * AMR_E_INVALID before any device work */
int amr_tone8_symbols_at_host(amr_tone8_plan *plan, const void *x, int dtype, int64_t n_streams, int64_t x_stride,
                              const int64_t *offset, const int64_t *shift, double *Y);
/* the score and maximum stage alone on given window energies P
 * [n_streams][n_win][15 + 2 search] (column li is line c2 - search + li): the
 * start slots are j < n_win - 48; start = j* T; score may be NULL */
int amr_tone8_peak_host(int64_t T, int64_t search, const double *P, int64_t n_streams, int64_t n_win, int64_t *start,
                        int64_t *shift, double *score);
/* the slicer and soft stages alone on given Y [n_streams][n_sym][8][2]: words
 * [n_streams][max(1, ceil(3 n_sym / 32))] (MSB first), soft [n_streams][3 n_sym]
 * (every bit from 0) */
int amr_tone8_slice_host(const double *Y, int64_t n_streams, int64_t n_sym, uint32_t *words);
int amr_tone8_soft_host(const double *Y, int64_t n_streams, int64_t n_sym, int8_t *soft);
/* tone8_modulate: the integer phase p in units of 1 / (2 L) cycle, p_0 = 0,
 * p_{k+1} = (p_k + L * inc_k) % (2 L), inc_k = c2 + 2 tone_k; sample i of symbol
 * k is float32(Sn[(p_k + i * inc_k) % (2 L)]), Sn [2 L] the caller's sine table,
 * so the output is the restatement's bit for bit.  A frame of an n_bytes
 * payload is (7 + ceil(8 n_bytes / 3)) * L samples; out / pcm / n_out as
 * amr_modulate_host. */
int amr_tone8_modulate_host(int64_t L, int64_t c2, const double *Sn, const uint8_t *data, int64_t data_stride,
                            const int64_t *n_bytes, int64_t n, float *out, int64_t out_stride, int64_t n_out,
                            int16_t *pcm, int64_t pcm_stride);

/* ---- benchmark / test input generator (no reference counterpart) ----------
 * d_out[s][i] = d_base[(s + row_offset) % n_base][i] + sigma * N(0,1), float32,
 * the deviate hashed from (seed, s, i): distinct noisy batches over the same
 * clean frames, generated in HBM (bench.py's in-flight batches).  Synchronous. */
int amr_synth_tile_noise(const float *d_base, int64_t n_base, int64_t n_samples, float *d_out, int64_t n_streams,
                         int64_t row_offset, float sigma, uint64_t seed);

/* ---- multi-GPU: RCCL over xGMI ----------------------------------------------- */
#define AMR_UNIQUE_ID_BYTES 128
int amr_comm_unique_id(uint8_t *id /* AMR_UNIQUE_ID_BYTES */);
int amr_comm_create(amr_comm **comm, const uint8_t *id, int nranks, int rank, int device);
int amr_comm_destroy(amr_comm *comm);
/* ncclAllGather of bytes_per_rank bytes per rank, on the comm's own stream in
 * call order (safe with several plans in flight); with a plan it is ordered
 * after the plan's queued work, and the plan's later work waits for it before
 * writing any output (its filters overlap the gather); the plan's
 * synchronize waits for it too. */
int amr_allgather(amr_comm *comm, const void *d_send, void *d_recv, int64_t bytes_per_rank,
                  amr_psk_plan *plan);
/* the same, ordered after / before the FSK plan's queued work */
int amr_fsk_allgather(amr_comm *comm, const void *d_send, void *d_recv, int64_t bytes_per_rank,
                      amr_fsk_plan *plan);
int amr_comm_synchronize(amr_comm *comm);
/* Host-memory collectives of the sharded host path (multi.py RcclTransport;
 * decoder.decode_from_buffer_batch with a transport): synchronous, on the
 * comm's stream behind its earlier gathers, through a device staging buffer
 * the comm keeps.  allgather_host: recv = world x bytes_per_rank, rank-major;
 * allreduce_max: values[i] = max over ranks (count doubles, in place); a
 * barrier is allreduce_max of one value. */
int amr_comm_allgather_host(amr_comm *comm, const void *send, void *recv, int64_t bytes_per_rank);
int amr_comm_allreduce_max(amr_comm *comm, double *values, int64_t count);
int amr_comm_world(const amr_comm *comm, int *nranks, int *rank);

#ifdef __cplusplus
}
#endif
#endif /* AMR_H */
