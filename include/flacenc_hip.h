/*
 * flacenc_hip.h -- C ABI of the MI355X (gfx950) implementation of flacenc-rs's
 * per-subframe quantised-LPC analysis path and of the stages either side of it.
 *
 * Three levels, each a superset of the one before:
 *   candidates   flacenc_hip_qlpc_batch / _stereo_qlpc_batch   (coding::estimated_qlpc)
 *                flacenc_hip_fixed_lpc_batch                   (coding::fixed_lpc)
 *   frames       flacenc_hip_encode_stereo_frames / _encode_frames   (coding::encode_frame: the
 *                candidates plus encode_subframe and try_stereo_coding on the device)
 *   bytes        flacenc_hip_pack_stereo_frames / _pack_frames (Frame::write, both CRCs),
 *                flacenc_hip_encode_pack_*_frames_async (PCM in HBM -> frame bytes in one call),
 *                flacenc_hip_fill_le_bytes (packed interleaved PCM -> FrameBuf layout)
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point names the reference interface it replaces (paths relative
 * to the flacenc-rs v0.5.1 source tree).  The Rust-side binding a maintainer
 * would add is shown in INTEGRATION.md and shipped as source in rust/.
 *
 * Threading: a handle owns one HIP stream, its device scratch and its window
 * cache; it is NOT thread-safe -- use one handle per host thread / per GPU,
 * like the reference's per-thread `reusable!` scratch (src/lib.rs:92-116).
 * ONE STREAM AT A TIME PER HANDLE: the *_async entry points take a stream per call, but the handle's scratch
 * (and the marked-subframe counters its clean-up launches alternate between) is shared by all of them: calls
 * on one handle must be ordered on one stream (or by events) -- two streams need two handles.
 * Launch size: every count of units a call takes (subframes, frames, frames x channels, rows) is at most 2^31 - 1;
 * flacenc_hip_encode_[pack_]stereo_frames count four candidate subframes per frame, so at most (2^31 - 1) / 4
 * frames; flacenc_hip_fill_le_bytes takes at most 65535 frames per call (a grid dimension).  More is
 * FLACENC_HIP_ERR_BAD_ARGUMENT with nothing written.  Strides, offsets and buffer sizes are size_t / uint64_t, so
 * rows, records, frame bytes and table offsets may lie beyond 2^32 bytes of the pointer they are counted from.
 * DESIGN.md, "Launch size and address range", lists which entry points the test suite holds there, at which
 * sizes (2^31 / 2^32 bytes, 2^31 / 2^32 elements), and which it does not.
 * Errors never unwind across this boundary: every call returns an int status
 * (0 = OK, negative = error) and per-subframe `status` fields carry the
 * conditions on which the reference would panic.
 */
#ifndef FLACENC_HIP_H_
#define FLACENC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6: without a summation-order flag the autocorrelation is the stable build's on every shape (round 5: certified on blocks
 *    of 4096 / 4608 at orders up to 12; round 6: the reference's chains in a pass of their own everywhere else) -- other bytes
 *    for the same config than revision 5 on a fraction of a per mille of subframes; the product library exports the
 *    declarations of this header and nothing else (the debug hooks live in libflacenc_hip_hooks.so).  No signature changed.
 * 5: blocks of 4096 / 8192 / 16384 samples at orders from 16 sum in the stable build's order by default (other bytes
 *    for the same config than revision 4); the two flacenc_hip_debug_* symbols left the public ABI; new exports
 *    flacenc_hip_frame_wire_bytes, flacenc_hip_stereo_frame_wire_async, flacenc_hip_stream_offsets_async (round 4) and
 *    the flacenc_hip_comm_* / flacenc_hip_allgather_* collective calls (round 5).
 * 4: use_direct_mse / mae_optimization_steps in flacenc_hip_qlpc_config, NIGHTLY_SUM_ORDER, frame-level calls take
 *    blocks below 64 samples */
#define FLACENC_HIP_ABI_VERSION 6

/* FLAC allows LPC order 32; the reference's config verifier caps it at 24
 * (src/constant.rs:118, src/config.rs:304).  Orders 25..32 are an extension
 * and are rejected unless FLACENC_HIP_FLAG_ALLOW_ORDER_32 is set. */
#define FLACENC_HIP_MAX_LPC_ORDER 32
#define FLACENC_HIP_REF_MAX_LPC_ORDER 24
#define FLACENC_HIP_MAX_PRECISION 15      /* src/constant.rs qlpc::MAX_PRECISION */
#define FLACENC_HIP_MAX_RICE_PARAMETER 30 /* src/constant.rs:143 */
#define FLACENC_HIP_MAX_MAE_STEPS 64    /* (the reference has no bound; its experimental preset uses 20, src/config.rs:535) */
#define FLACENC_HIP_MIN_BLOCK_SIZE 64     /* MIN_BLOCK_SIZE_FOR_PREDICTION, src/constant.rs:51 */
#define FLACENC_HIP_MAX_BLOCK_SIZE 32767  /* src/constant.rs:57 */
#define FLACENC_HIP_MAX_RICE_PARTITIONS 256 /* 2^8: finest order for any block <= 32767 */
#define FLACENC_HIP_MAX_FIXED_LPC_ORDER 4   /* src/constant.rs:95 */

/* return codes */
#define FLACENC_HIP_OK 0
#define FLACENC_HIP_ERR_BAD_CONFIG (-1)   /* -> EncodeError::Config(VerifyError), src/error.rs:458 */
#define FLACENC_HIP_ERR_BAD_ARGUMENT (-2)
#define FLACENC_HIP_ERR_DEVICE (-3)       /* HIP runtime failure; see flacenc_hip_last_error */
#define FLACENC_HIP_ERR_UNSUPPORTED (-4)
#define FLACENC_HIP_ERR_NO_DEVICE (-5)

/* per-subframe status bits (the reference panics on these) */
#define FLACENC_HIP_SUBFRAME_OK 0
#define FLACENC_HIP_SUBFRAME_NONFINITE 1  /* assert at src/lpc.rs:786-799 */
#define FLACENC_HIP_SUBFRAME_NEG_ENERGY 2 /* assert at src/lpc.rs:646-655 */

/* config::Window, src/config.rs:344-359 */
#define FLACENC_HIP_WINDOW_RECTANGLE 0
#define FLACENC_HIP_WINDOW_TUKEY 1
/* Extra analysis windows of FLACENC_HIP_FLAG_WINDOW_SEARCH only (flacenc_hip_set_lpc_windows); the config's
 * window_type keeps rejecting them.  Pieces of a block of n samples: s = (start * n) >> 16, e = (end * n) >> 16 in 64-bit
 * integers; T(m) = the reference's Tukey weights of length m with the entry's alpha (lpc::window_weights, src/lpc.rs:96-120),
 * all zeros for m < 2.
 *   PARTIAL_TUKEY:  T(e - s) on [s, e), zero elsewhere;
 *   PUNCHOUT_TUKEY: T(s) on [0, s), zero on [s, e), T(n - e) on [e, n). */
#define FLACENC_HIP_WINDOW_PARTIAL_TUKEY 2
#define FLACENC_HIP_WINDOW_PUNCHOUT_TUKEY 3
#define FLACENC_HIP_MAX_LPC_WINDOWS 8      /* the config's window + at most 7 extra windows */
#define FLACENC_HIP_WINDOW_UNIT 65536      /* start / end of an extra window: fractions of the block in 1/65536 */

#define FLACENC_HIP_FLAG_ALLOW_ORDER_32 1u
/* Build extension, NOT a reference mode (the reference always runs the exhaustive search,
 * src/rice.rs:246-298): keep the finest Rice partition order instead of merging down to order 0 --
 * BASELINE config 2's "fixed Rice partition order".  Output stays valid, lossless FLAC; it is just
 * not the partition the reference would pick when a coarser order is cheaper. */
#define FLACENC_HIP_FLAG_FINEST_RICE_ORDER 2u
/* Kernel selection overrides (no reference counterpart; every choice produces identical results):
 * GENERIC_KERNEL keeps block-4096 / order <= 12 launches off the fused wave-per-subframe kernel;
 * FUSED_PACK / TWO_STAGE_PACK force flacenc_hip_encode_pack_stereo_frames_async's one-kernel or
 * two-kernel form (default: two kernels, the faster choice measured since the deciding kernels run at
 * three workgroups per CU). */
#define FLACENC_HIP_FLAG_GENERIC_KERNEL 4u
#define FLACENC_HIP_FLAG_FUSED_PACK 8u
#define FLACENC_HIP_FLAG_TWO_STAGE_PACK 16u
/* Autocorrelation in the summation order of the reference's stable build: one sequential mul_add chain
 * per lag over t = order .. n-1 (weighted_auto_correlation_nosimd, src/lpc.rs:533-548), computed one
 * subframe per lane by a kernel of its own, instead of the kernels' own orders (a chain per lane or per 16-sample
 * chunk, combined by a tree -- same FMA count, different roundings; certified against the reference's on the fused
 * kernel's shapes, see FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER below and DESIGN.md section 2).
 * With this flag R[], the LPC coefficients and therefore every integer output are those of the stable
 * reference build for everything the oracle pins.  Costs one extra pass over the samples.
 * The flag also reaches the path's other order-sensitive sum: with OrderSel::ApproxEnt, fixed_lpc's
 * estimator takes every partition's sum of |e| from find_sum_abs_f32 (src/arrayutils.rs:496-506), which in
 * the stable build is one sequential f32 chain per partition; a kernel that gives a lane one (subframe,
 * partition) pair reproduces those chains for the five orders, so the selector's keys -- and with them the
 * chosen candidate and the frame bytes of the reference's default configuration -- are the stable
 * build's, 24-bit material included (tests/test_gpu_reference_order.py). */
#define FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER 32u
/* The same two sums in the order of the reference's `simd-nightly` build -- the build its published numbers and
 * compression ratios come from (report/report.nightly.md).  Autocorrelation (weighted_auto_correlation_simd,
 * src/lpc.rs:510-531 over weighted_delay_prod_sum_impl :439-500): per lag 8 (lags 0..7) or 16 (lags 8..15)
 * strided f64 lane chains over the 64-byte-aligned body of the windowed buffer, a scalar chain over head and
 * foot, an ordered lane sum.  find_sum_abs_f32 (src/arrayutils.rs:459-506): 16 f32 lane chains + head / foot.
 * Defined up to lpc_order 15 only: from lag 16 on the vectors are 128 / 256 bytes wide and where `as_simd`
 * splits the buffer depends on the allocator; flacenc_hip_verify_config answers ERR_UNSUPPORTED there, and
 * BAD_CONFIG if both order flags are set. */
#define FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER 64u

/* The kernels' own order as it is.  Without a summation-order flag, blocks of 4096 / 4608 samples at orders up to 12 (the
 * fused kernel's shapes) are CERTIFIED: the kernels keep their own autocorrelation sums where a perturbation bound on the
 * Toeplitz solve, held against the distance of every coefficient to its rounding boundary, says that the quantised LPC
 * parameters equal those of the reference's sequential chains, and recompute the subframe from those chains where it
 * does not (DESIGN.md section 2 lists what of the bound is shown and what is assumed and measured: it is evidence-backed,
 * not a theorem about the floating-point recursion; systems the recursion does not find positive definite are never
 * certified) -- so that every integer output (coefficients, shift, order, residual,
 * Rice partition, bit counts, frame bytes) is the stable build's, at the chunk tree's speed on material that is not
 * strongly tonal.  On material that IS (music, mostly: the certificate's second tier and the recomputation are serial
 * work), launches that return integers only -- no autocorr, no lpc_coefs -- switch, by what the certificate's counters
 * said about the launches before them (a verdict per 4096 subframes or more), to two passes (the reference's chains for every
 * subframe on the matrix cores, then the fused kernel): the same integers at a flat 1.4 x the certified kernel's best
 * time; a choice of speed, never of result ("the order mode by material").
 * EVERY OTHER SHAPE takes those two passes always (round 6; the pass of chains in front of whatever kernel takes the
 * shape -- an order certificate inside the small blocks' kernel was up to 140 x slower on music): there the unflagged R[],
 * coefficients and integers are the stable build's outright.
 * This flag switches the certificate -- and the other shapes' pass of reference chains -- off (blocks of 4096 / 8192 /
 * 16384 at orders from 16 keep the chains: they cost nothing extra there): a valid encoding of the same configuration
 * whose coefficients may differ from the reference's in the last quantisation step on a fraction of a per mille of
 * subframes. */
#define FLACENC_HIP_FLAG_CANONICAL_SUM_ORDER 128u

/* A modifier of FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER for callers that consume the INTEGER outputs only (a drop-in under
 * encode_with_fixed_block_size does: QuantizedParameters, residuals, Rice partitions, frame bytes): shapes whose unflagged
 * order is certified to give the stable build's integers (blocks of 4096 / 4608 samples at orders up to 12) keep it -- no
 * second pass over the samples there -- and every other shape takes the stable build's chains as the flag alone would.
 * What is given up is only the bit-equality of the optional floating-point outputs (autocorr, lpc_coefs). */
#define FLACENC_HIP_FLAG_INTEGER_PARITY_ONLY 256u

/* Wasted bits (RFC 9639 section 11.25), an extension like FLACENC_HIP_FLAG_FINEST_RICE_ORDER: the reference never writes
 * them (its parser asserts the flag is 0, src/component/parser.rs:446-448).  Per subframe signal x of width w (a role L,
 * R, M, S of a stereo frame -- S at bits_per_sample + 1 -- or a channel of an Independent(n) frame):
 *   - use_constant and x constant: today's Constant, k = 0;
 *   - otherwise k = the trailing zero bits of the OR of all samples (0 when that OR is 0); for k > 0 the candidate is
 *     encode_subframe(x >> k, w - k) -- kind, predictor, residual and Rice partition of the shifted signal at the
 *     reduced width -- and its bit count that subframe's count_bits + k (the unary count is k - 1 zeros and a one);
 *     try_stereo_coding compares these counts as it does without the flag.
 * The result records keep their layout: flacenc_hip_stereo_frame_result::pad[c] is output channel c's k and
 * flacenc_hip_channel_result::pad[0] the channel's k; bits[] include the + k; the record and the residual row are
 * those of the shifted signal.  Every writer stores 0 there without the flag, and the packers read pad as k: callers
 * of flacenc_hip_pack_* that build records themselves must pass 0 in pad unless they mean wasted bits.
 * Honoured by the frame-level calls (flacenc_hip_encode_[stereo_]frames[_async], flacenc_hip_encode_pack_*_async,
 * flacenc_hip_encode_pcm[_stereo], flacenc_hip_encode_variable[_async]); the candidate-level batches
 * (flacenc_hip_qlpc_batch, _stereo_qlpc_batch, _fixed_lpc_batch) answer FLACENC_HIP_ERR_UNSUPPORTED.  FUSED_PACK is
 * ignored under this flag (a kernel choice, never a result).
 * A flagged call first scans every frame for wasted bits and then SYNCHRONISES the stream once to read how many frames
 * have some: the *_async forms block the host for that long, and a flagged call cannot be captured into a graph.  Frames
 * without wasted bits take exactly the unflagged kernels; frames with some are analysed again, as shifted signals, by
 * the candidate batches, and a deciding kernel writes their records over the first pass's.
 * Scratch: for m such frames the handle holds m * rows shifted rows, and as many LPC and (with use_fixed) fixed-LPC
 * candidate rows, each row ceil4(block_size) int32 (rows = 4 for stereo frames, else channels) -- 3 x 6.4 GB (+ 25 %
 * growth slack) when all 98 304 stereo frames of 4096 samples are marked; memory that stays with the handle until
 * flacenc_hip_destroy.  Callers that bound memory bound the frames per call. */
#define FLACENC_HIP_FLAG_WASTED_BITS 512u

/* LPC order search, an extension like FLACENC_HIP_FLAG_WASTED_BITS (libFLAC searches the order; the reference always codes
 * lpc_order coefficients, src/coding.rs:360-381).  For every LPC candidate subframe with lpc_order = P (a role L, R, M, S
 * of a stereo frame, a channel, or a row of a candidate batch):
 *   - R[0..P] is the autocorrelation FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER gives (the stable build's chains), or the
 *     simd-nightly build's with FLACENC_HIP_FLAG_NIGHTLY_SUM_ORDER; CANONICAL_SUM_ORDER and INTEGER_PARITY_ONLY have no
 *     effect under this flag;
 *   - candidate o = 1..P: the recursion on R[0..o] with levinson_quantize's status checks on lags 0..o,
 *     quantize_parameters, the residual and the reference's exhaustive Rice search (max_rice_parameter and
 *     FINEST_RICE_ORDER honoured); its key is the exact Lpc::count_bits;
 *   - the candidate with status 0 and the smallest key is coded, the lower order on a tie; if no order has status 0 the
 *     record is the order-P record, status included.
 * The record and residual row are the chosen order's (order = o after quantize_parameters' tail-zero truncation),
 * `autocorr` holds R[0..P], `lpc_coefs` the chosen order's unquantised coefficients with zeros from o on.  Candidate P is
 * the REFERENCE_SUM_ORDER record, so no flagged LPC record -- and, since encode_subframe and try_stereo_coding compare
 * exact bit counts, no flagged frame -- is longer than the REFERENCE_SUM_ORDER one; at lpc_order 1 no byte changes.
 * Honoured by the candidate batches (flacenc_hip_qlpc_batch[_async], _stereo_qlpc_batch[_async]) and every frame-level
 * call, which then take the candidate batches and the stand-alone deciding kernels for every shape; composes with
 * FLACENC_HIP_FLAG_WASTED_BITS; FUSED_PACK is ignored; flacenc_hip_fixed_lpc_batch accepts and ignores the flag.
 * use_direct_mse with this flag answers FLACENC_HIP_ERR_UNSUPPORTED (flacenc_hip_verify_config and every call).
 * Scratch: P predictor records of 144 bytes per subframe (about 0.7 GB for 393 216 subframes at order 12), kept by the
 * handle until flacenc_hip_destroy. */
#define FLACENC_HIP_FLAG_ORDER_SEARCH 1024u

/* LPC window search (libFLAC's apodization), an extension like FLACENC_HIP_FLAG_ORDER_SEARCH: every LPC candidate subframe
 * with lpc_order = P (a role, a channel, a row of a candidate batch, a shifted row under WASTED_BITS) is analysed under
 * W windows and the shortest result is coded.  Window 0 is the config's (window_type, tukey_alpha); windows 1 .. W-1 are
 * the handle's extra windows (flacenc_hip_set_lpc_windows; W <= FLACENC_HIP_MAX_LPC_WINDOWS).  A fresh handle holds five:
 *   PARTIAL_TUKEY(0.2) [0, 36044), PARTIAL_TUKEY(0.2) [29492, 65536), PUNCHOUT_TUKEY(0.2) [0, 21845),
 *   PUNCHOUT_TUKEY(0.2) [21845, 43690), PUNCHOUT_TUKEY(0.2) [43690, 65536)   (in FLACENC_HIP_WINDOW_UNIT)
 * -- shaped after libFLAC's partial_tukey(2) and punchout_tukey(3), not its weights.
 *   - R_j[0..P] is the autocorrelation of the signal under window j in the stable build's order (the simd-nightly build's
 *     with NIGHTLY_SUM_ORDER); CANONICAL_SUM_ORDER and INTEGER_PARITY_ONLY have no effect under this flag;
 *   - the candidates are (j, P) for every window j -- with FLACENC_HIP_FLAG_ORDER_SEARCH (j, o) for every j and o = 1..P --
 *     each built from R_j as ORDER_SEARCH builds one from R[] (status checks, quantize_parameters, residual, exhaustive
 *     Rice search), keyed by the exact Lpc::count_bits;
 *   - the candidate with status 0 and the smallest key is coded, ties to the lower window, then the lower order; if none
 *     has status 0, candidate (0, P), status included.
 * The record and residual row are the winner's, `autocorr` its window's R[0..P], `lpc_coefs` its unquantised coefficients
 * with zeros from o on.  Candidate (0, P) is the REFERENCE_SUM_ORDER record (NIGHTLY_SUM_ORDER's under that flag), so no
 * flagged record or frame is longer than that call's -- nor, with ORDER_SEARCH as well, than the ORDER_SEARCH call's.  With
 * no extra window every output and launch is that of the same call with REFERENCE_SUM_ORDER (or NIGHTLY_SUM_ORDER) in
 * this flag's place, or with ORDER_SEARCH set of the ORDER_SEARCH call.  The extra-window list has no effect without the
 * flag.  Honoured where ORDER_SEARCH is (candidate batches, every frame-level call; composes with WASTED_BITS; FUSED_PACK
 * ignored; flacenc_hip_fixed_lpc_batch accepts and ignores it); use_direct_mse with this flag answers
 * FLACENC_HIP_ERR_UNSUPPORTED.  No host synchronisation: a flagged call is capturable wherever the ORDER_SEARCH call is
 * (the first call at a new block size builds the extra windows' weights, as every first call does the config's).
 * Scratch: 264 B per (subframe, window) for R[] and 144 B per (subframe, candidate); the handle runs the search over slices
 * of subframes that keep it at or below 768 MiB (1 GiB with the handle's growth slack) whatever n, W and P are -- this
 * bound covers FLACENC_HIP_FLAG_ORDER_SEARCH as well.  Extra windows' weights (4 bytes per sample and block size) stay in
 * the handle's window cache until flacenc_hip_destroy. */
#define FLACENC_HIP_FLAG_WINDOW_SEARCH 2048u

/* Guided LPC order search (libFLAC's default mode; only its -e codes every order as FLACENC_HIP_FLAG_ORDER_SEARCH does):
 * the order of every LPC candidate subframe is guessed from the prediction error the Levinson recursion leaves at each
 * order, and only the guesses are coded.  Inputs per subframe with lpc_order = P: n, the block size; w, the row's bits per
 * sample as the key uses it (bits_per_sample + 1 for the side role, w - k for a shifted row under WASTED_BITS); q,
 * quant_precision; K, the handle's guesses per window (flacenc_hip_set_order_guesses; a fresh handle holds 1).  For every
 * window j, R = R_j[0..P] exactly as WINDOW_SEARCH defines it (without WINDOW_SEARCH j = 0 is the only window): the stable
 * build's order, or nightly's under NIGHTLY_SUM_ORDER; CANONICAL_SUM_ORDER and INTEGER_PARITY_ONLY have no effect.
 *   1. k_o, o = 1..P: unquantised coefficient number o - 1 of ORDER_SEARCH's candidate o on R[0..o] (all coefficients are
 *      zero when R[0] = 0).
 *   2. e_0 = R[0]; e_o = e_(o-1) * (1.0 - k_o * k_o) in binary64, the multiply, the subtraction and the multiply each
 *      rounded on their own (no fma).
 *   3. Order o is eligible iff for every i <= o candidate i has status 0 and e_i >= 0 (a NaN fails); the first failure
 *      ends the chain.
 *   4. x_o = (float)(e_o * (0.5 / (double)n)); b_o = 0.5f * log2f(x_o) if x_o > 0 and that value is > 0, else +0.0f
 *      (libm's log2f).
 *   5. cost_o = (double)b_o * (double)(n - o) + (double)(o * (q + w)), multiply and add each rounded on their own.
 *   6. The guesses of window j are the K eligible orders with the smallest (cost_o, o); fewer when fewer are eligible.
 *   7. The candidates are (0, P) and every guess (j, o), each built and keyed exactly as ORDER_SEARCH / WINDOW_SEARCH build
 *      and key a candidate; the one with status 0 and the smallest exact Lpc::count_bits is coded, ties to the lower
 *      window, then the lower order; with no such candidate (0, P), status included.
 * The record and residual row are the winner's, `autocorr` its window's R[0..P], `lpc_coefs` its unquantised coefficients
 * with zeros from o on.  The candidates are a subset of the exhaustive search's and contain the REFERENCE_SUM_ORDER
 * record (NIGHTLY_SUM_ORDER's under that flag): no flagged record or frame is longer than that call's, none shorter than
 * the same call with ORDER_SEARCH in this flag's place; when every order with status 0 is eligible and K covers them every
 * output is that ORDER_SEARCH call's; at lpc_order 1 without extra windows no byte differs from the REFERENCE_SUM_ORDER
 * call.  With ORDER_SEARCH the flag answers FLACENC_HIP_ERR_BAD_CONFIG, with use_direct_mse FLACENC_HIP_ERR_UNSUPPORTED
 * (flacenc_hip_verify_config and every call).  WINDOW_SEARCH with an empty extra-window list plus this flag is this flag's
 * call.  Honoured where ORDER_SEARCH is (candidate batches, every frame-level call; composes with WASTED_BITS; FUSED_PACK
 * ignored; flacenc_hip_fixed_lpc_batch accepts and ignores it).  No host synchronisation: a flagged call is capturable
 * wherever the ORDER_SEARCH call is.
 * Scratch: ORDER_SEARCH's (264 B per (subframe, window), 144 B per (subframe, window, order)) and 8 B more per (subframe,
 * window, order) for k_o, inside the same 768 MiB slice bound. */
#define FLACENC_HIP_FLAG_ORDER_GUESS 4096u

/* LPC coefficient precision search (libFLAC's -p, do_qlp_coeff_prec_search), an extension like the three flags above: an
 * LPC subframe pays order x precision bits for its coefficients whatever its length, so every LPC candidate subframe with
 * lpc_order = P and quant_precision = q0 (a role, a channel, a row of a candidate batch, a shifted row under WASTED_BITS)
 * is coded at the precisions q_i = q0 - i, i = 0 .. Q-1, and the shortest result is kept.  F is the handle's floor
 * (flacenc_hip_set_precision_floor; a fresh handle holds 5, libFLAC's FLAC__MIN_QLP_COEFF_PRECISION): Q = q0 - F + 1 when
 * F < q0, else 1.
 *   - the candidates are (j, o, i): (j, o) ranges exactly over what the other flags define -- (0, P) alone; every order
 *     under ORDER_SEARCH; every window under WINDOW_SEARCH; (0, P) and each window's K guesses under ORDER_GUESS, whose
 *     guesses are computed as without this flag (its cost formula keeps q = q0) -- and each kept (j, o) is coded at every
 *     q_i;
 *   - candidate (j, o, i) is the recursion on R_j[0..o] with the status checks, as under those flags (R_j in the stable
 *     build's order, nightly's under NIGHTLY_SUM_ORDER; CANONICAL_SUM_ORDER and INTEGER_PARITY_ONLY have no effect), then
 *     quantize_parameters(a, q_i) on the unquantised coefficients -- which do not depend on i --, the residual and the
 *     exhaustive Rice search (max_rice_parameter and FINEST_RICE_ORDER honoured), keyed by the exact Lpc::count_bits with
 *     q_i in the precision term;
 *   - the candidate with status 0 and the smallest key is coded, ties to the lower window, then the lower order, then the
 *     higher precision; if none has status 0, candidate (0, P, q0), status included.
 * The record and residual row are the winner's and record.precision is its q_i; `autocorr` and `lpc_coefs` are as the other
 * search flags define them.  Candidate (0, P, q0) is the REFERENCE_SUM_ORDER record (NIGHTLY_SUM_ORDER's under that flag),
 * so no flagged record or frame is longer than that call's, nor than the same call without this flag when other search
 * flags are set.  Unlike the order search, bytes do change at lpc_order 1.  With F >= q0 every output and launch is that of
 * the same call without this flag: of the call with REFERENCE_SUM_ORDER (or NIGHTLY_SUM_ORDER) in its place when no other
 * search flag remains.  The floor has no effect without the flag.  Honoured where ORDER_SEARCH is (candidate batches,
 * every frame-level call; composes with WASTED_BITS, ORDER_SEARCH, WINDOW_SEARCH and ORDER_GUESS; FUSED_PACK ignored;
 * flacenc_hip_fixed_lpc_batch accepts and ignores it); use_direct_mse with this flag answers FLACENC_HIP_ERR_UNSUPPORTED
 * (flacenc_hip_verify_config and every call).  No host synchronisation: a flagged call is capturable wherever the
 * ORDER_SEARCH call is.
 * Scratch: 144 B per (subframe, window, order, precision) in place of ORDER_SEARCH's 144 B per (subframe, window, order),
 * inside the same 768 MiB slice bound; k_o stays 8 B per (subframe, window, order). */
#define FLACENC_HIP_FLAG_PRECISION_SEARCH 8192u

/* Escaped Rice partitions (RFC 9639 section 9.2.7.1), an extension like FLACENC_HIP_FLAG_WASTED_BITS: the reference never
 * escapes (its parser reads the escape code as a parameter, src/component/parser.rs:653-690).  A partition may be stored
 * as raw two's-complement samples of a 5-bit-coded width instead of Rice codes: 9 bits for a partition of digital silence,
 * and never more than the container for noise.
 * Record encoding: rice_params[q] = 0x80 | w marks partition q as escaped with raw width w, 0..31; values 0..30 stay Rice
 * parameters; bits 5 and 6 of a marked byte are zero.  The record's size and wire form do not change.
 * Definition, for one candidate record with status 0: residual row e, warm-up length o = record.order, block size n,
 * max_p = max_rice_parameter.
 *   1. F = finest_partition_order(n, max(64, o)) (src/rice.rs:157-165).  At level r = F .. 0 partition q covers
 *      [max(q * (n >> r), o), (q + 1) * (n >> r)) and holds cnt samples.
 *   2. R_r(q), the Rice cost, is what the unflagged search computes: PrcBitTable::from_errors(.., 4) at level F with its
 *      clamps, merge(.., 4) below it, minimizer(max_p).
 *   3. w_r(q), the raw width, is the smallest w with -2^(w-1) <= e < 2^(w-1) for every e of the partition; 0 when all
 *      are zero or cnt = 0; a merged partition's width is the larger of its children's.
 *   4. E_r(q) = 4 + 5 + cnt * w when w <= 31; a partition of width 32 cannot be escaped.
 *   5. A partition is escaped iff E < R -- strictly: a tie stays Rice.
 *   6. A level costs sum_q min(R, E); the walk is the reference's (src/rice.rs:277-291): from F, to a coarser level only
 *      on a strictly smaller cost.  FLACENC_HIP_FLAG_FINEST_RICE_ORDER evaluates level F alone.
 *   7. rice_order is the chosen level, rice_params its parameters or marks, code_bits its cost, sum_quotients the exact
 *      sum of z >> k over the NON-escaped partitions, subframe_bits the exact count: everything in front of the residual
 *      as Lpc::count_bits / FixedLpc::count_bits have it, then 2 + 4 + sum_q (pb + (escaped ? 5 + cnt * w :
 *      sum(z >> k) + cnt * (k + 1))) with pb = 5 iff some NON-escaped parameter exceeds 14.  The escape code is 0b1111
 *      under pb = 4 and 0b11111 under pb = 5.
 * Consequences: a record in which no partition escapes is byte for byte the unflagged record (a level's flagged cost never
 * exceeds its unflagged cost and both walks keep the finest level among the minima, so a chosen level without escapes is
 * the unflagged choice); no flagged record or frame is longer than the same call's without the flag; records with
 * status != 0 are left untouched.
 * Honoured by the candidate batches (flacenc_hip_qlpc_batch[_async], _stereo_qlpc_batch[_async], _fixed_lpc_batch[_async]):
 * a pass behind their kernels rewrites the five fields of the records they return; residual rows, `autocorr`,
 * `lpc_coefs`, the selector keys of flacenc_hip_fixed_lpc_batch and the fixed order it selects are unchanged (the
 * BitCount selector keeps comparing unescaped code_bits).  ORDER_SEARCH / WINDOW_SEARCH / ORDER_GUESS / PRECISION_SEARCH
 * choose their winner by the unescaped key as without this flag, and the pass then runs on the winner's record:
 * searching with escaped keys is not done.  The frame-level calls (flacenc_hip_encode_[stereo_]frames[_async],
 * flacenc_hip_encode_pack_*_async, flacenc_hip_encode_pcm[_stereo], flacenc_hip_encode_variable[_async]) take the
 * candidate batches and the stand-alone deciding kernels for every shape under this flag -- it trades the fused kernels
 * for the general path -- and the deciding kernels compare the updated subframe_bits (the fixed candidate's selector key
 * is held against the Verbatim size as without the flag).  FUSED_PACK is ignored.  Blocks below 64 samples have no
 * candidates: their frames are the unflagged call's.  Composes with WASTED_BITS (the shifted rows go through the same
 * batches), use_direct_mse and every summation-order flag.  No host synchronisation of its own.  The packers need no
 * flag: they write marked records of any origin (see "The packers' domain" below). */
#define FLACENC_HIP_FLAG_RICE_ESCAPE 16384u

/* where the caller's sample / output buffers live */
#define FLACENC_HIP_MEM_HOST 0
#define FLACENC_HIP_MEM_DEVICE 1

typedef struct flacenc_hip_handle flacenc_hip_handle;

/* The fields of config::Qlpc (src/config.rs:271-288) and config::Prc
 * (src/config.rs:211-214) that parameterise the path.  Defaults: order 10,
 * precision 15, Tukey(0.4), max_parameter 30 (src/constant.rs:109-115,
 * src/config.rs:216-221).
 * `use_direct_mse` / `mae_optimization_steps` (src/config.rs:280, :285; both off by default) select the
 * reference's EXPERIMENTAL estimators in perform_qlpc (src/coding.rs:333-351): the covariance-method LPC of
 * LpcEstimator::weighted_lpc_with_direct_mse (src/lpc.rs:853-903: weighted_lagged_outer_prod_sum :573-600, a
 * Cholesky solve with a doubling diagonal regulariser) and, with steps > 0, its IRLS re-weighting towards the
 * mean absolute error (lpc_with_irls_mae, :814-850; steps is ignored unless use_direct_mse is set, as there).
 * The reference's stable `Verify` rejects both switches outside its `experimental` feature (config.rs:302-326);
 * this ABI follows the experimental build.  Its linear solver is nalgebra's (not part of the reference tree):
 * results equal the oracle's restatement of nalgebra 0.32's published algorithm bit for bit, and the oracle's
 * solution solves the covariance method's exact system to rounding; what cannot be pinned is bit-equality with
 * nalgebra itself.  mae_optimization_steps is limited to
 * FLACENC_HIP_MAX_MAE_STEPS.  A block of block_size <= lpc_order samples (nothing to estimate from, lpc.rs:542, :587)
 * never reaches these estimators: the candidate batches answer FLACENC_HIP_ERR_BAD_ARGUMENT for every
 * block_size < 64, the frame-level calls code such blocks as Constant or Verbatim (coding.rs:396). */
typedef struct flacenc_hip_qlpc_config {
  uint32_t lpc_order;          /* 1..=24 (..=32 with ALLOW_ORDER_32) */
  uint32_t quant_precision;    /* 1..=15 */
  uint32_t window_type;        /* FLACENC_HIP_WINDOW_* */
  float tukey_alpha;           /* 0.0..=1.0 */
  uint32_t max_rice_parameter; /* ..=30 */
  uint32_t flags;
  uint32_t use_direct_mse;         /* 0 / 1 */
  uint32_t mae_optimization_steps; /* 0..=FLACENC_HIP_MAX_MAE_STEPS */
} flacenc_hip_qlpc_config;

/* One record per analysed subframe: everything `estimated_qlpc`
 * (src/coding.rs:360-381) returns inside SubFrame::Lpc except the residual
 * samples (written separately) and the warm-up samples (= the first `order`
 * input samples).  Fixed size (352 bytes) so that records can be all-gathered
 * across GPUs as-is.
 *   coefs/order/shift/precision = component::QuantizedParameters
 *                                 (src/component/datatype.rs:2164-2170)
 *   rice_order/rice_params      = component::Residual partition_order / rice_params
 *                                 (src/component/datatype.rs:2269-2284)
 *   code_bits                   = rice::PrcParameter::code_bits (src/rice.rs:220-224)
 *   sum_quotients               = Residual::sum_quotients (datatype.rs:2325-2331)
 *   subframe_bits               = BitRepr for Lpc::count_bits (src/component/bitrepr.rs:492-499)
 */
typedef struct flacenc_hip_subframe_params {
  int16_t coefs[32];
  uint8_t order;
  int8_t shift;
  uint8_t precision;
  uint8_t rice_order;
  int32_t status;
  uint64_t code_bits;
  uint64_t subframe_bits;
  uint64_t sum_quotients;
  uint8_t rice_params[FLACENC_HIP_MAX_RICE_PARTITIONS];
} flacenc_hip_subframe_params;

/* ---- lifetime --------------------------------------------------------- */
int flacenc_hip_abi_version(void);
int flacenc_hip_device_count(void);
/* Replaces the per-thread scratch set-up of the reference (`reusable!`
 * LPC_ESTIMATOR src/lpc.rs:916, WINDOW_CACHE :219, QLPC_ERROR_BUFFER
 * src/coding.rs:353, PRC_FINDER src/rice.rs:301). */
int flacenc_hip_create(flacenc_hip_handle** out, int device_id);
void flacenc_hip_destroy(flacenc_hip_handle* h);
const char* flacenc_hip_last_error(const flacenc_hip_handle* h);

/* config::Qlpc::verify + config::Prc::verify, src/config.rs:302-326, 224-229 */
int flacenc_hip_verify_config(const flacenc_hip_qlpc_config* cfg);

/* lpc::window_weights (src/lpc.rs:96-120), evaluated on the host in f32 with
 * libm cosf exactly as the reference does; this is the table the kernels use. */
int flacenc_hip_window_weights(const flacenc_hip_qlpc_config* cfg, uint32_t block_size, float* out);

/* FLACENC_HIP_FLAG_WINDOW_SEARCH: the handle's extra analysis windows, entry i = (types[i], alphas[i], starts[i], ends[i]),
 * n_extra <= FLACENC_HIP_MAX_LPC_WINDOWS - 1 (0: the config's window only).  FLACENC_HIP_ERR_BAD_CONFIG for an unknown
 * type, an alpha outside [0, 1] (NaN included), for PARTIAL_ / PUNCHOUT_TUKEY start >= end or end > 65536, n_extra > 7,
 * or NULL arrays with n_extra > 0; a rejected call leaves the list as it was.  start / end are ignored for RECTANGLE and
 * TUKEY.  Takes effect for the calls enqueued after it; the list travels with no call that lacks the flag. */
int flacenc_hip_set_lpc_windows(flacenc_hip_handle* h, const uint32_t* types, const float* alphas,
                                const uint32_t* starts, const uint32_t* ends, uint32_t n_extra);
/* FLACENC_HIP_FLAG_ORDER_GUESS: K, the guesses per window, 1..=32 (else FLACENC_HIP_ERR_BAD_ARGUMENT, the value kept); a
 * fresh handle holds 1.  Read when a call is enqueued: it applies to the calls made after it, and has no effect without
 * the flag. */
int flacenc_hip_set_order_guesses(flacenc_hip_handle* h, uint32_t k);
/* FLACENC_HIP_FLAG_PRECISION_SEARCH: F, the lowest precision searched, 1..=15 (else FLACENC_HIP_ERR_BAD_ARGUMENT, the
 * value kept); a fresh handle holds 5.  Read when a call is enqueued: it applies to the calls made after it, and has no
 * effect without the flag. */
int flacenc_hip_set_precision_floor(flacenc_hip_handle* h, uint32_t floor);
/* The deepest FLAC stream the decode calls take: 24 (a fresh handle) or 32 bits per sample (else
 * FLACENC_HIP_ERR_BAD_ARGUMENT, the value kept).  At 32, flacenc_hip_decode_frames / _verify_frames / _index_frames /
 * _decode_pcm / _decode_streams / _decode_streams_md5 / _decode_ranges / _decode_ranges_planar / _recover_streams and
 * their _async and device forms accept bits_per_sample 4..=32 (bytes_per_sample >= ceil(bits / 8) as before), a frame
 * header may say 32 bits (sample-size code 7, or code 0 on a 32-bit stream), and the 33-bit side channel of a 32-bit
 * stereo frame is reconstructed in 64-bit arithmetic.  Every decoded value of a valid stream fits 32 bits; on an invalid
 * stream that passes both CRCs a frame of more than 24 bits decodes to the low 32 bits of the two's-complement 64-bit
 * computation.  A float32 element of flacenc_hip_decode_ranges_planar at more than 24 bits is float(v), rounded to
 * nearest even, times 2^-(bits - 1): not exact, and it can equal 1.0.  At 24 every call behaves as it always has: more
 * than 24 bits is FLACENC_HIP_ERR_UNSUPPORTED for the call and FLACENC_HIP_DECODE_UNSUPPORTED for a frame.  Read when a
 * call is enqueued.  The encode calls do not read it: flacenc_hip_set_max_encode_bits_per_sample is theirs. */
int flacenc_hip_set_max_bits_per_sample(flacenc_hip_handle* h, uint32_t bits);
/* The deepest PCM the stream-level encode calls take: 24 (a fresh handle) or 32 bits per sample (else
 * FLACENC_HIP_ERR_BAD_ARGUMENT, the value kept); independent of flacenc_hip_set_max_bits_per_sample.  At 32,
 * flacenc_hip_encode_pcm / _encode_pcm_stereo, flacenc_hip_encode_streams and flacenc_hip_encode_streams_planar
 * (FLACENC_HIP_SAMPLE_I32 only) accept bits_per_sample 25..=32 at bytes_per_sample 4, and a stream or class of more
 * than 24 bits runs the step of flacenc_hip_encode_pack_frames_wide (below) in place of the frame-level calls; streams of 24
 * bits or fewer launch the kernels they always have.  At 24 every call answers as it always has.  Read when a call is
 * enqueued.  The frame-level record calls, the candidate batches and flacenc_hip_encode_variable stay at 24 bits. */
int flacenc_hip_set_max_encode_bits_per_sample(flacenc_hip_handle* h, uint32_t bits);
/* The weights of one extra-window entry over a block of block_size (<= 32767) samples, on the host: no handle, no GPU.
 * The same validation as flacenc_hip_set_lpc_windows (FLACENC_HIP_ERR_BAD_CONFIG). */
int flacenc_hip_lpc_window_weights(uint32_t type, float alpha, uint32_t start, uint32_t end, uint32_t block_size,
                                   float* out);

/* ---- the hot path ----------------------------------------------------- */
/*
 * Batched `estimated_qlpc` (src/coding.rs:360-381): for k in 0..n_subframes the
 * subframe is the `block_size` samples at `samples + k*stride` (the layout of
 * FrameBuf::channel_slice, src/source.rs:251-253, batched).  Requires
 * 64 <= block_size <= 32767 (blocks < 64 never reach the path, coding.rs:396; the frame-level calls
 * flacenc_hip_encode_[stereo_]frames / pack_* take them -- 1 <= block_size -- and run encode_subframe's
 * `too_short` branch: Constant or Verbatim only).
 *   bps[k]        bits per sample of subframe k (8..=25; side channels carry +1,
 *                 src/coding.rs:444); only enters subframe_bits.
 *   params[k]     output record (see above)
 *   residual      output, subframe k at residual + k*residual_stride; first
 *                 `order` slots are zero (src/lpc.rs:349)
 *   autocorr      optional [n_subframes][33] f64: R[0..=lpc_order] (src/lpc.rs:780-785)
 *   lpc_coefs     optional [n_subframes][32] f64: unquantised coefficients (src/lpc.rs:792-796)
 *   memory_kind   FLACENC_HIP_MEM_HOST: all pointers are host memory, the call
 *                 stages through the handle's device scratch and returns after
 *                 the results are back on the host.
 *                 FLACENC_HIP_MEM_DEVICE: all pointers are device memory on the
 *                 handle's GPU; the call returns after the kernel completed.
 */
int flacenc_hip_qlpc_batch(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                           const int32_t* samples, size_t n_subframes, uint32_t block_size,
                           size_t stride, const uint8_t* bps,
                           flacenc_hip_subframe_params* params, int32_t* residual,
                           size_t residual_stride, double* autocorr, double* lpc_coefs,
                           int memory_kind);

/* Same with device pointers only, enqueued on `stream` (a hipStream_t; NULL =
 * HIP's default stream) without synchronising. */
int flacenc_hip_qlpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                 const int32_t* samples, size_t n_subframes, uint32_t block_size,
                                 size_t stride, const uint8_t* bps,
                                 flacenc_hip_subframe_params* params, int32_t* residual,
                                 size_t residual_stride, double* autocorr, double* lpc_coefs,
                                 void* stream);

/*
 * The four `estimated_qlpc` calls `encode_frame` makes for a 2-channel frame
 * (src/coding.rs:530-544): encode_frame_impl(Independent(2)) on L and R, then
 * try_stereo_coding's MidSide frame on M = (l + r) >> 1 and S = l - r
 * (src/coding.rs:476-491).  `frames` is batched FrameBuf layout
 * (src/source.rs:115-127): channel c of frame f at frames + (2f + c)*stride.
 * M and S are formed on the GPU.  Outputs are indexed 4f + {0:L, 1:R, 2:M, 3:S};
 * the S record's subframe_bits uses bits_per_sample + 1 (src/coding.rs:444).
 * This is the candidate-level call: all four records and residual rows come back and the choice between
 * L+R / L+S / R+S / M+S (src/coding.rs:493-522) is the caller's.  flacenc_hip_encode_stereo_frames below makes
 * it on the GPU (with the fixed-LPC candidate) and returns only the two chosen rows.
 */
int flacenc_hip_stereo_qlpc_batch(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                  const int32_t* frames, size_t n_frames, uint32_t block_size,
                                  size_t stride, uint32_t bits_per_sample,
                                  flacenc_hip_subframe_params* params, int32_t* residual,
                                  size_t residual_stride, int memory_kind);
int flacenc_hip_stereo_qlpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_qlpc_config* cfg,
                                        const int32_t* frames, size_t n_frames, uint32_t block_size,
                                        size_t stride, uint32_t bits_per_sample,
                                        flacenc_hip_subframe_params* params, int32_t* residual,
                                        size_t residual_stride, void* stream);

/* ---- encode_frame for 2-channel frames, decision on the device ------------------------ */
/*
 * config::Encoder fields that steer `encode_frame` (src/coding.rs:530-544): SubFrameCoding's
 * candidate switches (src/config.rs:167-183), its config::Fixed (src/config.rs:236-244: max_order
 * and OrderSel, :400-409) and StereoCoding (src/config.rs:137-144).  Reference defaults: every
 * switch on, fixed_max_order 4, ApproxEnt with 16 partitions (src/constant.rs:35, :95).
 */
#define FLACENC_HIP_ORDERSEL_BITCOUNT 0  /* OrderSel::BitCount: code every order, count the bits */
#define FLACENC_HIP_ORDERSEL_APPROXENT 1 /* OrderSel::ApproxEnt { partitions } (the default) */
/* ApproxEnt feeds estimate_entropy (src/coding.rs:200-227) the partition's sum of |e| as an f32.  Here that
 * is the exact integer sum rounded to f32 once; the reference accumulates in f32 (find_sum_abs_f32,
 * src/arrayutils.rs:496: one sequential chain in the stable build, 16 lanes in simd-nightly).  All three
 * coincide while the sum stays below 2^24 and differ by f32 rounding above it (24-bit material, loud 16-bit
 * material at higher fixed orders): without FLACENC_HIP_FLAG_REFERENCE_SUM_ORDER the selected fixed order --
 * and hence the frame bytes -- are then not guaranteed identical to a CPU build's; with it the sums are the
 * stable build's sequential chains, bit for bit.  BitCount has no such dependence. */

typedef struct flacenc_hip_frame_config {
  flacenc_hip_qlpc_config qlpc;
  uint32_t use_constant;
  uint32_t use_fixed;
  uint32_t use_lpc;
  uint32_t use_leftside;
  uint32_t use_rightside;
  uint32_t use_midside;
  uint32_t fixed_max_order;  /* 0..=4 */
  uint32_t fixed_order_sel;  /* FLACENC_HIP_ORDERSEL_* */
  uint32_t fixed_partitions; /* ApproxEnt.partitions */
  uint32_t reserved;
} flacenc_hip_frame_config;

#define FLACENC_HIP_KIND_CONSTANT 0 /* SubFrame::Constant */
#define FLACENC_HIP_KIND_VERBATIM 1 /* SubFrame::Verbatim */
#define FLACENC_HIP_KIND_FIXED 2    /* SubFrame::FixedLpc */
#define FLACENC_HIP_KIND_LPC 3      /* SubFrame::Lpc */

/* What `encode_frame` decides for one stereo frame: `try_stereo_coding`'s channel assignment
 * (src/coding.rs:493-522; 0 Independent(2), 1 LeftSide, 2 RightSide, 3 MidSide), and for each of
 * the two output channels (ChannelAssignment::select_channels, datatype.rs:1173-1185) which of
 * L, R, M, S it is (`role` 0..3), which SubFrame variant `encode_subframe` picked (`kind`), the
 * Constant's value, and the predictor record when kind == LPC or FIXED.  A FixedLpc subframe's
 * record holds FIXED_LPC_COEFS[order] (src/component/decode.rs:179-185) with shift 0 and
 * precision 0, the Rice partition of its error signal, and FixedLpc::count_bits
 * (src/component/bitrepr.rs:473-477) in subframe_bits.  `bits` are SubFrame::count_bits of the
 * four candidates L, R, M, S after encode_subframe. */
typedef struct flacenc_hip_stereo_frame_result {
  uint8_t channel_assignment;
  uint8_t kind[2];
  uint8_t role[2];
  uint8_t analysis_status; /* OR of the FLACENC_HIP_SUBFRAME_* bits of the four LPC analyses (L, R, M, S): non-zero
                              where the reference panics (lpc.rs:646, :786-799); the frame is still valid FLAC --
                              the affected candidate was dropped -- but a drop-in should raise */
  uint8_t pad[2];          /* pad[c]: wasted bits k of output channel c (FLACENC_HIP_FLAG_WASTED_BITS; 0 without it) */
  int32_t dc_offset[2];
  uint64_t bits[4];
  flacenc_hip_subframe_params lpc[2];
} flacenc_hip_stereo_frame_result;

/*
 * `encode_frame` (src/coding.rs:530-544) for a batch of 2-channel frames with the whole decision
 * on the GPU: L, R, M, S analysed, `encode_subframe` (coding.rs:384-418) applied to each,
 * `try_stereo_coding` picks the assignment, and only the two chosen residual rows are written:
 * residual + (2f + c)*residual_stride for output channel c of frame f (the LPC residual or the
 * fixed-LPC error signal, warm-up slots zero; all zeros for Constant / Verbatim).
 * With use_fixed the other input of encode_subframe, `fixed_lpc` (src/coding.rs:298-331:
 * reset_fixed_lpc_errors :182-197, estimate_entropy :200-227, select_order_and_encode_residual
 * :230-288), runs on the GPU too, so the whole default-configuration decision is on the device.
 * Block size 4096 with lpc_order <= 12, 16-byte aligned rows and power-of-two ApproxEnt.partitions
 * runs as ONE fused kernel (a wave per candidate, samples read from HBM once, losing candidates never
 * leave the CU); so do blocks of 256 / 512 / 1024 / 2048 and 288 / 576 / 1152 / 2304 samples (4 .. 32 finest Rice
 * partitions: several frames per workgroup) with the ApproxEnt selector and estimator partitions of a quarter,
 * half or whole number of those; blocks of 8192 / 16384 samples (and 4096 from order 13) take two analysing
 * passes and a deciding store pass; every other shape (any block size 64..32767, any order, any partition
 * count) runs the candidate batches into handle scratch followed by a controller kernel -- same outputs.
 */
/* Precondition (the reference checks it in FrameBuf::verify_samples, src/source.rs:262-275, before the path
 * is reached): every sample lies in [-2^(bits_per_sample-1), 2^(bits_per_sample-1)).  The frame entry points
 * do not re-check it; out-of-range samples give frames whose warm-up / Verbatim fields are truncated to
 * bits_per_sample bits.  The same precondition holds for every entry point that takes a width (`bps` /
 * `bits_per_sample`, 8..25 bits with the side channel): the fixed-LPC order selector's per-lane sums (v_sad_u32 on
 * biased values) are exact for such samples only, and out-of-width input may select a different fixed order on
 * power-of-two blocks than on ragged ones.  The big-block residual kernel checks each row's extremes against its
 * declared width (its byte planes carry no more) and sends an out-of-width subframe to the generic kernel instead. */
int flacenc_hip_encode_stereo_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                     const int32_t* frames, size_t n_frames, uint32_t block_size,
                                     size_t stride, uint32_t bits_per_sample,
                                     flacenc_hip_stereo_frame_result* results, int32_t* residual,
                                     size_t residual_stride, int memory_kind);
int flacenc_hip_encode_stereo_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                           const int32_t* frames, size_t n_frames, uint32_t block_size,
                                           size_t stride, uint32_t bits_per_sample,
                                           flacenc_hip_stereo_frame_result* results, int32_t* residual,
                                           size_t residual_stride, void* stream);

/* ---- fixed_lpc as a stand-alone batch (any block size, any channel count) ---------------- */
#define FLACENC_HIP_LAYOUT_SUBFRAMES 0     /* unit = one subframe at samples + k*stride */
#define FLACENC_HIP_LAYOUT_STEREO_FRAMES 1 /* unit = one 2-channel frame; outputs 4f + {L, R, M, S} */
/*
 * `fixed_lpc` (src/coding.rs:298-331) for a batch: reset_fixed_lpc_errors (:182-197), the order
 * selector of cfg->fixed_* (select_order_and_encode_residual :230-288; ApproxEnt partitions may
 * be any 1..=64 here) and the Rice-coded error signal of the selected order.  Only the fixed_* and
 * qlpc.max_rice_parameter fields of `cfg` are used.  Per subframe:
 *   params[k]        order = selected fixed order, coefs = FIXED_LPC_COEFS[order]
 *                    (src/component/decode.rs:179-185), shift 0, precision 0, the Rice partition,
 *                    code_bits, sum_quotients, subframe_bits = FixedLpc::count_bits (bitrepr.rs:473-477)
 *   residual         the order's error signal, first `order` slots zero
 *   selector_keys[k] optional: the selector's key of the selected order (estimate_entropy +
 *                    bps*order, or bps*order + code_bits for BitCount).  `fixed_lpc` returns Some(..)
 *                    iff this key is < baseline_bits (coding.rs:262, :284): that comparison, and
 *                    encode_subframe's choice (coding.rs:384-418), stay with the caller.
 *   bps              per-subframe bits per sample (SUBFRAMES layout; NULL -> bits_per_sample);
 *                    STEREO_FRAMES uses bits_per_sample (+1 for the side channel, coding.rs:444).
 * This is the general-shape companion of flacenc_hip_encode_stereo_frames, which fuses the same
 * computation into the frame decision for block_size 4096.
 */
int flacenc_hip_fixed_lpc_batch(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                const int32_t* samples, size_t n_units, uint32_t block_size, size_t stride,
                                const uint8_t* bps, uint32_t bits_per_sample, int layout,
                                flacenc_hip_subframe_params* params, int32_t* residual, size_t residual_stride,
                                uint64_t* selector_keys, int memory_kind);
int flacenc_hip_fixed_lpc_batch_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                      const int32_t* samples, size_t n_units, uint32_t block_size,
                                      size_t stride, const uint8_t* bps, uint32_t bits_per_sample, int layout,
                                      flacenc_hip_subframe_params* params, int32_t* residual,
                                      size_t residual_stride, uint64_t* selector_keys, void* stream);

/* ---- Frame::write on the GPU ---------------------------------------- */
/*
 * BitRepr::write for the frames flacenc_hip_encode_stereo_frames decided (src/component/bitrepr.rs:
 * Frame :289-319, FrameHeader :373-419 with fixed blocking and FrameOffset::Frame as
 * encode_fixed_size_frame sets it (src/coding.rs:581-606), Constant :449-454, Verbatim :463-470,
 * FixedLpc :479-487, Lpc :501-527, Residual :550-597; CRC_8_SMBUS over the header, CRC_16_UMTS over
 * the byte-aligned frame, :39-40).  Inputs are the outputs of flacenc_hip_encode_stereo_frames plus
 * its input samples (warm-up and Verbatim bodies); frame f gets frame number
 * first_frame_number + f*frame_number_step (step > 1 when frames were dealt round-robin over GPUs).
 *   out       frame f's bytes at out + f*out_stride; out_stride >= flacenc_hip_stereo_frame_bytes_bound
 *             (a multiple of 16; out 16-byte aligned); bytes beyond out_len[f] are unspecified
 *   out_len   [n_frames] byte length of each frame = Frame::count_bits / 8 (bitrepr.rs:275-287)
 * The frame is assembled in LDS: frames whose worst case (flacenc_hip_*_frame_bytes_bound) exceeds
 * 150 KiB -- e.g. 8 channels x 16384 samples x 24 bits -- are FLACENC_HIP_ERR_UNSUPPORTED.
 * sample_rate / bits_per_sample go into the header specs exactly as encode_frame_impl chooses them
 * (src/coding.rs:431-436); a rate or size without a code becomes "Unspecified".
 *
 * The packers' domain, for callers that build or move records themselves (flacenc_hip_pack_frames alike).  Nothing
 * of it is checked on the device:
 *   - a record describes a subframe the project's decoder reads (flacenc_hip_decode_frames);
 *   - order <= block_size >> rice_order: the first Rice partition may be empty (its parameter is still written),
 *     never negative;
 *   - rice_params[0 .. 2^rice_order) are Rice parameters 0..30, or 0x80 | w for a partition stored escaped at raw width
 *     w = 0..31 (FLACENC_HIP_FLAG_RICE_ESCAPE above; bits 5 and 6 zero): the escape code at the parameter width, the 5-bit
 *     width, then the partition's residuals in two's complement at w bits each; every residual of a marked partition
 *     fits its width; the residual is written with 5-bit parameters exactly when a NON-escaped parameter exceeds 14;
 *   - shift 0..15 and precision 1..15 (LPC); a Fixed record holds FIXED_LPC_COEFS[order], shift 0, precision 0;
 *   - every sample fits its width (bits_per_sample, + 1 for the side role, - pad[c] wasted bits) and every residual
 *     an int32; the residual row is that of the shifted signal, its first `order` slots are not read;
 *   - bits[] are the exact SubFrame::count_bits (+ pad[c]), and over a frame they sum to at most
 *     channels * (8 + block_size * bits_per_sample): the LDS image is sized from flacenc_hip_*_frame_bytes_bound plus a
 *     few words, and a frame beyond it would be written outside the image.
 */
size_t flacenc_hip_stereo_frame_bytes_bound(uint32_t block_size, uint32_t bits_per_sample);
int flacenc_hip_pack_stereo_frames(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames,
                                   uint32_t block_size, size_t stride,
                                   const flacenc_hip_stereo_frame_result* results, const int32_t* residual,
                                   size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                   uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                                   size_t out_stride, uint32_t* out_len, int memory_kind);
int flacenc_hip_pack_stereo_frames_async(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames,
                                         uint32_t block_size, size_t stride,
                                         const flacenc_hip_stereo_frame_result* results, const int32_t* residual,
                                         size_t residual_stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                         uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out,
                                         size_t out_stride, uint32_t* out_len, void* stream);

/* ---- encode_frame / Frame::write for Independent(channels) frames: mono and multi-channel -- */
/* What encode_subframe (src/coding.rs:384-418) decided for one channel of an Independent(n) frame
 * (encode_frame for channels != 2, src/coding.rs:537-541): the SubFrame variant, the Constant's
 * value, SubFrame::count_bits and the predictor record when kind == LPC or FIXED.  368 bytes. */
typedef struct flacenc_hip_channel_result {
  uint8_t kind; /* FLACENC_HIP_KIND_* */
  uint8_t analysis_status; /* FLACENC_HIP_SUBFRAME_* bits of this channel's LPC analysis (see above) */
  uint8_t pad[2];          /* pad[0]: wasted bits k of the channel (FLACENC_HIP_FLAG_WASTED_BITS; 0 without it); pad[1] 0 */
  int32_t dc_offset;
  uint64_t bits;
  flacenc_hip_subframe_params params;
} flacenc_hip_channel_result;

/*
 * encode_frame for frames of 1..8 independent channels (no stereo decorrelation: 2-channel
 * streams should use flacenc_hip_encode_stereo_frames).  `frames` is batched FrameBuf layout:
 * channel c of frame f at frames + (f*channels + c)*stride; results and residual rows use the same
 * index f*channels + c.  Candidates are computed as by flacenc_hip_qlpc_batch /
 * flacenc_hip_fixed_lpc_batch (handle scratch), then encode_subframe's choice runs on the GPU.
 */
int flacenc_hip_encode_frames(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                              const int32_t* frames, size_t n_frames, uint32_t channels, uint32_t block_size,
                              size_t stride, uint32_t bits_per_sample, flacenc_hip_channel_result* results,
                              int32_t* residual, size_t residual_stride, int memory_kind);
int flacenc_hip_encode_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                    const int32_t* frames, size_t n_frames, uint32_t channels,
                                    uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                    flacenc_hip_channel_result* results, int32_t* residual,
                                    size_t residual_stride, void* stream);
/* Frame::write for those frames; arguments as flacenc_hip_pack_stereo_frames. */
size_t flacenc_hip_frame_bytes_bound(uint32_t channels, uint32_t block_size, uint32_t bits_per_sample);
int flacenc_hip_pack_frames(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                            uint32_t block_size, size_t stride, const flacenc_hip_channel_result* results,
                            const int32_t* residual, size_t residual_stride, uint32_t bits_per_sample,
                            uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                            uint8_t* out, size_t out_stride, uint32_t* out_len, int memory_kind);
int flacenc_hip_pack_frames_async(flacenc_hip_handle* h, const int32_t* frames, size_t n_frames, uint32_t channels,
                                  uint32_t block_size, size_t stride, const flacenc_hip_channel_result* results,
                                  const int32_t* residual, size_t residual_stride, uint32_t bits_per_sample,
                                  uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                                  uint8_t* out, size_t out_stride, uint32_t* out_len, void* stream);

/*
 * encode_frame + Frame::write in one call, device pointers: PCM frames in, FLAC frame bytes out
 * (= flacenc_hip_encode_stereo_frames_async followed by flacenc_hip_pack_stereo_frames_async, same
 * arguments and outputs, no residual rows): the residual rows live in handle scratch between the two
 * kernels.  With FLACENC_HIP_FLAG_FUSED_PACK, block size 4096 and LPC order <= 12 it is ONE kernel: the
 * chosen residuals go from the deciding wave's registers straight into the frame's bit buffer in LDS and
 * never touch HBM (6 instead of 14 bytes of traffic per input sample, but fewer resident waves: slower).
 */
int flacenc_hip_encode_pack_stereo_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                                const int32_t* frames, size_t n_frames, uint32_t block_size,
                                                size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                                uint32_t first_frame_number, uint32_t frame_number_step,
                                                flacenc_hip_stereo_frame_result* results, uint8_t* out,
                                                size_t out_stride, uint32_t* out_len, void* stream);

/* The same for Independent(channels) frames: flacenc_hip_encode_frames_async +
 * flacenc_hip_pack_frames_async with the residual rows in handle scratch. */
int flacenc_hip_encode_pack_frames_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                         const int32_t* frames, size_t n_frames, uint32_t channels,
                                         uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                         uint32_t sample_rate, uint32_t first_frame_number,
                                         uint32_t frame_number_step, flacenc_hip_channel_result* results,
                                         uint8_t* out, size_t out_stride, uint32_t* out_len, void* stream);

/* The wide encode path: encode_frame + Frame::write for frames of 8..=32 bits per sample on
 * 64-bit integers, with the candidates of libFLAC's -0 .. -2.  Arguments as flacenc_hip_encode_pack_frames_async, without
 * the records; 2 channels take the stereo decision (the side channel has bits_per_sample + 1 bits, 33 at 32), any other
 * count is Independent.  out_stride >= flacenc_hip_stereo_frame_bytes_bound (2 channels) or flacenc_hip_frame_bytes_bound.
 * Device pointers; the call runs on the handle's stream and returns when the frames are written (there is no `stream`
 * argument and no _async form yet: the stream-level calls run the same step on their own streams).
 * Needs no opt-in: the caller names the path.  Per subframe (exact integers, no floating point):
 *   - Constant under use_constant; Verbatim for block_size < 64;
 *   - with use_fixed the fixed predictors of order 0..=min(fixed_max_order, 4): an order is eligible only if every
 *     residual lies in (-2^31, 2^31) (RFC 9639 section 9.2.7.3); per eligible order the exhaustive partitioned-Rice search
 *     (src/rice.rs:246-298 on exact 64-bit sums, parameters 0..=qlpc.max_rice_parameter); the smallest
 *     width * order + code_bits wins, ties to the lower order (OrderSel::BitCount, src/coding.rs:242-265); the subframe is
 *     Fixed if that key and its exact count_bits are below Verbatim's bits, with 5-bit (RICE2) parameters exactly when
 *     a parameter exceeds 14;
 *   - with FLACENC_HIP_FLAG_WASTED_BITS the subframe is that of x >> k at width - k bits, k counted as above;
 *   - try_stereo_coding (src/coding.rs:493-522) on the four exact bit counts.
 * NOT read on this path: use_lpc, every other field of cfg->qlpc, every search flag, FLACENC_HIP_FLAG_RICE_ESCAPE,
 * fixed_order_sel and fixed_partitions (ApproxEnt's f32 sums have no meaning at these magnitudes).  They are tolerated,
 * not refused: a batch may mix depths under one config.  The header's sample-size code is 7 for 32 bits and 0 for
 * 25..=31.  FLACENC_HIP_ERR_BAD_CONFIG for max_rice_parameter > 30 or fixed_max_order > 4. */
int flacenc_hip_encode_pack_frames_wide(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg,
                                        const int32_t* frames, size_t n_frames, uint32_t channels,
                                        uint32_t block_size, size_t stride, uint32_t bits_per_sample,
                                        uint32_t sample_rate, uint32_t first_frame_number,
                                        uint32_t frame_number_step, uint8_t* out, size_t out_stride,
                                        uint32_t* out_len);

/* Frame::count_bits / 8 (src/component/bitrepr.rs:275-287) of every frame from the decision records
 * alone: exactly the out_len flacenc_hip_pack_stereo_frames will produce.  Device pointers.  These
 * 4 bytes per frame are all an ordered multi-GPU gather has to exchange to place every frame in
 * the output stream (the role of ParSink, src/par.rs:67-95); the bytes themselves stay local. */
int flacenc_hip_stereo_frame_lengths_async(flacenc_hip_handle* h, const flacenc_hip_stereo_frame_result* results,
                                           size_t n_frames, uint32_t block_size, uint32_t bits_per_sample,
                                           uint32_t sample_rate, uint32_t first_frame_number,
                                           uint32_t frame_number_step, uint32_t* out_len, void* stream);

/* ParSink's reordering (src/par.rs:67-95: finished frames are put back into frame-number order for the
 * writer) for packed frames in HBM: frame i = lengths[i] bytes at src + src_offsets[i] is copied to
 * dst + dst_offsets[i].  Device pointers, any byte alignment.  Used twice by the multi-GPU gather of
 * packed frames: to compact a rank's strided pack output into one contiguous run for the RCCL
 * all-gather, and to place every rank's frames at their stream offsets afterwards. */
int flacenc_hip_place_frames_async(flacenc_hip_handle* h, const uint8_t* src, const uint64_t* src_offsets,
                                   const uint32_t* lengths, size_t n_frames, uint8_t* dst,
                                   const uint64_t* dst_offsets, void* stream);

/* The ordered gather's two device steps (what ParSink, src/par.rs:67-95, does with a BTreeMap on one host).
 * flacenc_hip_stereo_frame_wire_async turns this rank's decision records into their wire form -- the 48 bytes of frame
 * fields and, of each of the two 352-byte subframe records, the 96 fixed bytes + the first 2^finest_order Rice
 * parameters (src/rice.rs:157-165; the rest of rice_params[256] is always zero): flacenc_hip_frame_wire_bytes(block)
 * bytes, 368 of 752 for blocks of 4096 -- at wire + f * wire_stride, and in the same pass writes the frames' byte
 * lengths (flacenc_hip_stereo_frame_lengths_async's values) to out_len when that is not NULL.
 * flacenc_hip_stream_offsets_async takes the all-gathered lengths as the collective delivers them -- rank-major,
 * gathered_lengths[r * ceil(n / world) + j] = stream frame j * world + r, shorter ranks zero-padded; world = 1 is
 * plain stream order -- and writes, in stream order, offsets[f] = header_bytes + sum of the lengths of frames below f,
 * lengths_stream[f] (optional, NULL to skip) and total[0] = header_bytes + sum of all lengths. */
size_t flacenc_hip_frame_wire_bytes(uint32_t block_size);
int flacenc_hip_stereo_frame_wire_async(flacenc_hip_handle* h, const flacenc_hip_stereo_frame_result* results,
                                        size_t n_frames, uint32_t block_size, uint32_t bits_per_sample,
                                        uint32_t sample_rate, uint32_t first_frame_number, uint32_t frame_number_step,
                                        uint8_t* wire, size_t wire_stride, uint32_t* out_len, void* stream);
int flacenc_hip_stream_offsets_async(flacenc_hip_handle* h, const uint32_t* gathered_lengths, size_t n_frames_total,
                                     uint32_t world, uint64_t header_bytes, uint32_t* lengths_stream,
                                     uint64_t* offsets, uint64_t* total, void* stream);

/* ---- the collective of the ordered gather (one process per GPU) -------------------------------------------- */
/*
 * ParSink (src/par.rs:67-95) re-orders the frames its worker threads finish; with one PROCESS per GPU (frame f on
 * rank f mod world) that re-ordering needs one exchange, and this is it: an RCCL communicator owned by the handle
 * and an all-gather of fixed-size per-frame records on the caller's stream.  librccl is opened at run time on the
 * first of these calls (ERR_UNSUPPORTED when it cannot be found; FLACENC_HIP_RCCL names another path) -- a
 * single-GPU drop-in never loads it.
 *   flacenc_hip_comm_unique_id   ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to the other ranks by
 *                                whatever means the host has (a file, a socket, MPI, torch.distributed's store)
 *   flacenc_hip_comm_create      ncclCommInitRank on the handle's device; collective over all `world` ranks
 *   flacenc_hip_comm_info        rank / world of the handle's communicator (world = 0: none)
 *   flacenc_hip_allgather_async  ncclAllGather of bytes_per_rank bytes: recv[r * bytes_per_rank ..] = rank r's send
 *   flacenc_hip_allgather_records_async
 *                                the ordered gather's exchange for n_total frames dealt round-robin: `local` holds this
 *                                rank's n_local = ceil((n_total - rank) / world) records of record_bytes each (wire
 *                                records from flacenc_hip_stereo_frame_wire_async, or its 4-byte lengths); `gathered`
 *                                receives world * ceil(n_total / world) records rank-major -- record r * per_rank + j =
 *                                stream frame j * world + r, ranks one frame short zero-padded -- the layout
 *                                flacenc_hip_stream_offsets_async reads.  `local` may be the rank's own slot of
 *                                `gathered` (in place).  Device pointers; enqueued on `stream`.
 */
#define FLACENC_HIP_COMM_ID_BYTES 128
int flacenc_hip_comm_unique_id(uint8_t id[FLACENC_HIP_COMM_ID_BYTES]);
int flacenc_hip_comm_create(flacenc_hip_handle* h, const uint8_t id[FLACENC_HIP_COMM_ID_BYTES], int rank, int world);
int flacenc_hip_comm_destroy(flacenc_hip_handle* h);
int flacenc_hip_comm_info(flacenc_hip_handle* h, int* rank, int* world);
int flacenc_hip_allgather_async(flacenc_hip_handle* h, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int flacenc_hip_allgather_records_async(flacenc_hip_handle* h, const void* local, size_t n_local, size_t n_total,
                                        size_t record_bytes, void* gathered, void* stream);

/* ---- input side ------------------------------------------------------- */
/*
 * FrameBuf::fill_le_bytes (src/source.rs:288-298) for a run of consecutive frames of one stream, on
 * the GPU: le_bytes_to_i32s (src/arrayutils.rs:273-290; little-endian samples of 1..4 bytes, sign-
 * extended) and deinterleave (src/arrayutils.rs:248-264).  `bytes` holds `total_samples` inter-channel
 * samples of packed interleaved PCM starting at the first frame of the run; frame f, channel c goes
 * to frames + (f*channels + c)*stride, zero-filled beyond total_samples (the short last block).
 * Uploading packed 16- / 24-bit PCM and widening here halves (or better) the PCIe traffic of the
 * host-pointer paths; the MD5 of the input stays with the caller (src/source.rs:406-428).
 * At most 65535 frames per call (one grid row per frame): 65536 and more are FLACENC_HIP_ERR_BAD_ARGUMENT and
 * nothing is written; a longer stream is filled in runs.  `bytes` and `frames` may be of any size (8 channels x
 * 4 bytes x 65535 frames of 4096 samples are 8.6 GB in and out).
 */
int flacenc_hip_fill_le_bytes(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples,
                              uint32_t channels, uint32_t bytes_per_sample, size_t n_frames, uint32_t block_size,
                              int32_t* frames, size_t stride, int memory_kind);
int flacenc_hip_fill_le_bytes_async(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t total_samples,
                                    uint32_t channels, uint32_t bytes_per_sample, size_t n_frames,
                                    uint32_t block_size, int32_t* frames, size_t stride, void* stream);

/* ---- host-memory streaming path: what a drop-in under encode_with_fixed_block_size experiences ---- */
/*
 * Packed interleaved little-endian 2-channel PCM in host memory -> FLAC frame bytes in host memory, for a
 * whole stream (or a long run of it) in one call: the feed loop of the reference's par-mode encoder
 * (src/par.rs:288-325: fill a FrameBuf, hand it to a worker, collect the frame) with the GPU as the
 * worker pool.  The run is cut into chunks of whole frames; per chunk the packed PCM (2..3 bytes per sample
 * instead of 4) goes host -> device through pinned staging on a copy stream, flacenc_hip_fill_le_bytes +
 * flacenc_hip_encode_pack_stereo_frames run on the compute stream, the frames are compacted on the device
 * (flacenc_hip_place_frames) and exactly their bytes come back on a second copy stream -- two slots, so the
 * upload of chunk k + 1, the analysis of chunk k and the download of chunk k - 1 overlap.
 *   pcm            total_samples inter-channel samples, bytes_per_sample each, L R L R ...
 *   block_size     every frame has block_size samples except the last (total_samples % block_size; a last
 *                  block of fewer than 64 samples is coded as the reference codes it: encode_subframe skips
 *                  both predictors, `too_short` src/coding.rs:389-418, and emits Constant or Verbatim)
 *   out/out_len    frames back to back in frame order (what the stream writer appends after the
 *                  metadata blocks) and each frame's byte length; out_total = bytes written
 * `pcm` / `out` may be ordinary (pageable) memory -- then they are staged through the handle's pinned
 * buffers with a host memcpy -- or memory from flacenc_hip_host_alloc, which is transferred directly.
 * The MD5 of the input and STREAMINFO stay with the caller (src/source.rs:406-428); a caller that encodes many files
 * gets all their digests in one call from flacenc_hip_md5_spans.
 */
int flacenc_hip_encode_pcm_stereo(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                                  uint64_t total_samples, uint32_t bytes_per_sample, uint32_t bits_per_sample,
                                  uint32_t block_size, uint32_t sample_rate, uint32_t first_frame_number,
                                  uint32_t frame_number_step, uint8_t* out, size_t out_capacity, uint32_t* out_len,
                                  uint64_t* out_total);
/* The same for any channel count 1..=8 (samples interleaved c0 c1 .. c0 c1 ..): 2 channels as above, other
 * counts as Independent(channels) frames (src/coding.rs:537-541: flacenc_hip_encode_pack_frames_async). */
int flacenc_hip_encode_pcm(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                           uint64_t total_samples, uint32_t channels, uint32_t bytes_per_sample,
                           uint32_t bits_per_sample, uint32_t block_size, uint32_t sample_rate,
                           uint32_t first_frame_number, uint32_t frame_number_step, uint8_t* out, size_t out_capacity,
                           uint32_t* out_len, uint64_t* out_total);
/* page-locked host memory for the calls above (NULL on failure) */
void* flacenc_hip_host_alloc(size_t bytes);
void flacenc_hip_host_free(void* p);
/* Host threads (the caller's included) that share the staging copies of flacenc_hip_encode_pcm* when `pcm` or
 * `out` is pageable memory; 0 or 1 = the caller's thread alone, default 4.  The helper threads belong to the
 * handle, sleep between calls and end with flacenc_hip_destroy -- the counterpart of the reference's worker
 * threads feeding and draining FrameBufs (src/par.rs:288-325), which only move bytes here. */
int flacenc_hip_set_host_threads(flacenc_hip_handle* h, int threads);

/* ---- the way back: decode, verify and index frames on the GPU ----------------------------------------------- */
/*
 * Frame::decode (src/component/decode.rs:55-110) over the frames the parser reads (src/component/parser.rs: frame
 * :183, residual :633) -- what `flacenc decode` runs (flacenc-bin/src/main.rs:270-370) -- for a whole launch of frames
 * at once.  Frame f is lengths[f] bytes at bytes + offsets[f]: the strided pack output (offsets = f * out_stride,
 * lengths = out_len) and the stream flacenc_hip_stream_offsets_async places both fit.  RFC 9639 frames: both sync codes,
 * every block-size code (6 and 7 included) and sample-rate code, channel codes 0..10, sample-size code 0 (= the
 * stream's bits_per_sample), the coded number up to 7 bytes, CRC-8; Constant, Verbatim, Fixed 0..4 and LPC 1..32
 * (precision 1..15) subframes, wasted bits, both Rice methods and escaped partitions (raw width 0..31); left/side,
 * right/side and mid/side are undone as in decode.rs:71-98, and reconstruction accumulates in 64 bits and truncates to
 * i32 (decode.rs:159-177).
 * The decoder is a deliberate superset of the reference's parser in two places, neither of which affects a frame the
 * reference writes: it accepts wasted bits (the parser asserts there are none, parser.rs:446-448), and it reads an
 * escape code as an escaped partition (the parser reads it as a Rice parameter, parser.rs:653-690).
 *   out          channel-major int32, frame f channel c at out + (f*channels + c)*stride (the encoder's input layout,
 *                flacenc_hip_fill_le_bytes); stride >= max_block_size; samples beyond the block are zero
 *   block_sizes  the block size of the frame's header; numbers (NULL to skip): its coded frame or sample number
 *   status       0, or an OR of FLACENC_HIP_DECODE_*; a frame with a status has zero rows, block size 0, number 0
 * bits_per_sample must be 4..24 (32-bit FLAC needs a 33-bit side channel) and channels 1..8; a frame whose bit depth is
 * above 24 or whose block size is above max_block_size is UNSUPPORTED.  For any input bytes the decoder reads nothing
 * outside [offsets[f], offsets[f] + lengths[f]) and writes nothing outside frame f's rows and slots: garbage gives a
 * status, never a fault.  flacenc_hip_decode_frames also checks every span against n_bytes (LENGTH when it does not
 * fit) and takes host or device pointers; the *_async forms take device pointers and enqueue on `stream`.
 * flacenc_hip_verify_frames_async runs the same parse, compares every sample with `expected` (same layout as `out`)
 * and writes only `status` (MISMATCH on a frame that decodes to other samples): `flac --verify` for a whole launch.
 * flacenc_hip_index_frames_async finds the frames of a buffer that holds only frames (a .flac file after its metadata
 * blocks): every byte position whose header is valid for the stream with a matching CRC-8 is a candidate, each is
 * parsed for its length and CRC-16, and the frames are exactly those reachable from byte 0 by "the next frame starts
 * where this one ends" (resolved on the device by pointer jumping), so a header planted inside a frame is never one.
 * offsets / lengths receive at most max_frames frames in stream order; n_frames[0] = the number written, with
 * FLACENC_HIP_INDEX_ERROR set when that chain does not end exactly at n_bytes or holds more than max_frames frames, and
 * also when the buffer holds more candidate headers (planted ones included) than max_frames + max_frames / 4 + 4096, the
 * room of the candidate table: the candidates at the highest positions are then dropped and the chain may stop early.
 * A caller clears that by passing a larger max_frames.  With or without the flag the frames written are a verified prefix
 * of the chain: each passed its header checks and CRC-16 and starts where the one before it ends, the first at byte 0
 * (so a stream cut inside its last frame gives the frames before it), and nothing is written past that count.
 * Scratch (the per-frame skim records, the candidates) comes from the handle.
 */
#define FLACENC_HIP_DECODE_BAD_HEADER 1u       /* no sync code, a reserved code or a malformed coded number */
#define FLACENC_HIP_DECODE_HEADER_CRC 2u
#define FLACENC_HIP_DECODE_FRAME_CRC 4u
#define FLACENC_HIP_DECODE_PARSE 8u            /* a subframe or residual field out of range, or the frame ends early */
#define FLACENC_HIP_DECODE_LENGTH 16u          /* the parsed length differs from lengths[f] */
#define FLACENC_HIP_DECODE_STREAM_MISMATCH 32u /* channels or bit depth differ from the arguments (parser.rs:197-214) */
#define FLACENC_HIP_DECODE_UNSUPPORTED 64u     /* bit depth above 24 or block size above max_block_size */
#define FLACENC_HIP_DECODE_MISMATCH 128u       /* verify: a sample differs from `expected` */
#define FLACENC_HIP_INDEX_ERROR 0x8000000000000000ull
int flacenc_hip_decode_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, size_t n_frames, uint32_t channels,
                                    uint32_t bits_per_sample, uint32_t max_block_size, int32_t* out, size_t stride,
                                    uint32_t* block_sizes, uint64_t* numbers, uint32_t* status, void* stream);
int flacenc_hip_decode_frames(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                              const uint32_t* lengths, size_t n_frames, uint32_t channels, uint32_t bits_per_sample,
                              uint32_t max_block_size, int32_t* out, size_t stride, uint32_t* block_sizes,
                              uint64_t* numbers, uint32_t* status, int memory_kind);
int flacenc_hip_verify_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, const uint64_t* offsets,
                                    const uint32_t* lengths, size_t n_frames, uint32_t channels,
                                    uint32_t bits_per_sample, uint32_t max_block_size, const int32_t* expected,
                                    size_t stride, uint32_t* status, void* stream);
int flacenc_hip_index_frames_async(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, uint32_t channels,
                                   uint32_t bits_per_sample, size_t max_frames, uint64_t* offsets, uint32_t* lengths,
                                   uint64_t* n_frames, void* stream);

/*
 * Decoded rows to packed PCM: the inverse of flacenc_hip_fill_le_bytes (interleave + i32s_to_le_bytes), with one block
 * size per frame so that the rows of a variable-blocking stream pack back to back.
 *   frames          frame f, channel c is the row at frames + (f*channels + c)*stride: flacenc_hip_decode_frames' `out`
 *   block_sizes     samples of frame f; 0 is legal and contributes nothing (what the decoder leaves for a frame with a
 *                   status); a value above `stride` counts as `stride`, so garbage never reads outside a row
 *   out             with off[f] the exclusive prefix sum of the block sizes, sample i of frame f, channel c goes to
 *                   out + ((off[f] + i)*channels + c)*bytes_per_sample as the low bytes_per_sample bytes of its
 *                   two's-complement value, little-endian; a value that does not fit the width KEEPS ITS LOW BYTES (no
 *                   saturation, no status): the exact inverse of le_bytes_to_i32s for every value that fits
 *   sample_offsets  n_frames + 1 entries, NULL to skip: off[f], and the total in the last
 *   total           1 entry: the inter-channel samples of all frames
 * For the bytes_per_sample a stream's bit depth needs (ceil(bits / 8)) the output is the byte string the STREAMINFO MD5
 * is defined over (src/source.rs:406-428), and for 16 / 24 bits the WAV payload.
 * Nothing is read beyond block_sizes[f] samples of a row and no byte of `out` outside [0, total*channels*
 * bytes_per_sample) is written; when that range exceeds out_capacity NOTHING is written to `out`, `total` and
 * `sample_offsets` still are, and the call returns FLACENC_HIP_ERR_BAD_ARGUMENT.  channels 1..8,
 * bytes_per_sample 1..4, up to 2^31 - 1 frames (no limit of 65535 as in flacenc_hip_fill_le_bytes); `out` may be NULL
 * when out_capacity is 0.  Host or device pointers (memory_kind); with device pointers the call enqueues two launches on
 * the handle's stream (with sample_offsets NULL the offsets live in the handle's scratch) and returns when they have run.
 * There is no stream-taking form yet: inside the library the same two launches run stream-ordered behind each group of
 * flacenc_hip_decode_pcm.
 */
int flacenc_hip_pack_le_bytes(flacenc_hip_handle* h, const int32_t* frames, size_t stride, const uint32_t* block_sizes,
                              size_t n_frames, uint32_t channels, uint32_t bytes_per_sample, uint8_t* out,
                              uint64_t out_capacity, uint64_t* sample_offsets, uint64_t* total, int memory_kind);
/*
 * The mirror of flacenc_hip_encode_pcm: frame bytes in host memory in, packed interleaved little-endian PCM in host
 * memory out (the flacenc_hip_pack_le_bytes layout), in one call.  `bytes` holds only frames -- a .flac file after its
 * metadata blocks, or the output of flacenc_hip_encode_pcm / flacenc_hip_encode_variable --, `bytes` and `out` are
 * pageable or flacenc_hip_host_alloc memory.  The call decodes the verified chain of frames that starts at byte 0
 * (flacenc_hip_index_frames_async: header checks, CRC-8, CRC-16, each frame starting where the one before ends), writes
 * their samples to `out` back to back and stops at the first position where it cannot go on.  It returns
 * FLACENC_HIP_OK whenever the arguments were acceptable and the device worked; totals says how far it got:
 *   totals[0]  frames decoded            totals[1]  inter-channel samples written
 *   totals[2]  bytes of input consumed: the start of the frame it stopped at, or n_bytes
 *   totals[3]  why it stopped: 0, the chain ended exactly at n_bytes;
 *              FLACENC_HIP_DECODE_NO_ROOM, the next frame's samples do not fit in out_capacity (every frame before it is
 *              complete in `out`; a second call on bytes + totals[2] continues the stream, and the two outputs
 *              concatenated are the output of one call with enough room);
 *              FLACENC_HIP_DECODE_CHAIN, no verified frame starts at totals[2] (garbage, a corrupted frame, a stream cut
 *              inside a frame -- or a frame longer than flacenc_hip_frame_bytes_bound(channels, max_block_size,
 *              bits_per_sample), which no frame this library writes is);
 *              else the FLACENC_HIP_DECODE_* bits of a frame of the chain that decoded with a status.
 * In every case `out` beyond totals[1]*channels*bytes_per_sample bytes is untouched, and garbage in never faults.
 * channels 1..8; bits_per_sample 4..24 (else FLACENC_HIP_ERR_UNSUPPORTED); max_block_size 1..65536 (STREAMINFO's; a frame
 * above it stops the call with UNSUPPORTED); bytes_per_sample from ceil(bits_per_sample / 8) to 4; n_bytes == 0 returns OK
 * with all-zero totals.  Device memory and pinned staging are bounded whatever n_bytes and the decoded size are: the
 * input moves in windows of bytes (128 MiB; the upload of the next window does not wait for the index of this one), the
 * rows and the PCM in groups of frames (128 MiB / (max_block_size*channels*bytes_per_sample), 64..8192) over two slots
 * and the handle's three streams, with the staging copies of pageable buffers on the handle's host threads
 * (flacenc_hip_set_host_threads).  The bytes written and totals do not depend on that plan.
 */
#define FLACENC_HIP_DECODE_NO_ROOM 256u
#define FLACENC_HIP_DECODE_CHAIN 512u
int flacenc_hip_decode_pcm(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, uint32_t channels,
                           uint32_t bits_per_sample, uint32_t max_block_size, uint32_t bytes_per_sample, uint8_t* out,
                           uint64_t out_capacity, uint64_t totals[4]);

/*
 * A batch of streams in one call: what flacenc_hip_decode_pcm does for one stream, for every stream of a table, with a
 * number of kernel launches, synchronisations and transfers that does not depend on the number of streams -- the call
 * for a library of short files (a speech corpus, a sample pack, the tracks of an album), which otherwise pays the
 * decoder's fixed latency once per file.
 *   bytes, n_bytes   one buffer that holds every stream's frames.  Stream s is bytes [offset, offset + n_bytes) of it;
 *                    spans ascend by offset and never overlap, gaps between them are legal and are never read as frames
 *                    (whole .flac files back to back, each descriptor pointing behind that file's metadata blocks)
 *   streams          n_streams descriptors (struct flacenc_hip_stream_desc, 48 bytes each), ALWAYS host memory, read
 *                    before the call returns; channels, bits_per_sample, max_block_size and bytes_per_sample are the
 *                    stream's, as for flacenc_hip_decode_pcm
 *   out, out_bytes   one buffer for every stream's PCM: stream s owns the slot [out_offset, out_offset + out_capacity).
 *                    Slots must be disjoint; the library does NOT check that (overlapping slots give unspecified bytes
 *                    in the overlap, never a fault)
 *   totals           [n_streams][4]: per stream what flacenc_hip_decode_pcm's totals say
 *   call_totals      host memory in both kinds: [0] frames and [1] inter-channel samples decoded over all streams
 *   memory_kind      FLACENC_HIP_MEM_HOST (pageable or flacenc_hip_host_alloc memory) or FLACENC_HIP_MEM_DEVICE: where
 *                    bytes, out and totals live
 * For every stream the bytes in its slot and totals[s][0..3] are exactly what flacenc_hip_decode_pcm gives when called on
 * that stream alone with that slot as `out`: frames, samples, bytes consumed counted from the stream's own start, and the
 * stop reason (0, NO_ROOM, CHAIN, or a frame's status bits: UNSUPPORTED for a block above the stream's max_block_size).
 * A stream of 0 bytes gives all-zero totals.  Slot bytes beyond totals[s][1]*channels*bytes_per_sample and bytes of `out`
 * in no slot are untouched; garbage gives a stop reason, never a fault, and changes nothing for the other streams.  The one
 * difference: flacenc_hip_decode_pcm cuts its input into windows and therefore ends the chain at a frame longer than
 * flacenc_hip_frame_bytes_bound; the batch sees every stream whole and has no such limit.
 * max_frames bounds the frames of all chains together (at most 2^30; n_bytes / 9 + n_streams always suffices).
 * FLACENC_HIP_INDEX_ERROR
 * is set in call_totals[0] when the batch holds more chain frames than that, or more candidate headers than max_frames +
 * max_frames / 4 + 4096 (the rule of flacenc_hip_index_frames_async): then nothing is written to `out`, every stream's
 * totals are zero and the caller retries with a larger max_frames.
 * n_streams == 0 is OK.  FLACENC_HIP_ERR_BAD_ARGUMENT: a null pointer, n_streams above 2^24, max_frames above 2^30, spans
 * that do not ascend, overlap or reach past n_bytes, a slot that reaches past out_bytes, channels outside 1..8,
 * max_block_size outside 1..65536, bytes_per_sample above 4 or below ceil(bits_per_sample / 8);
 * FLACENC_HIP_ERR_UNSUPPORTED: a bits_per_sample outside 4..24.  In every error case nothing is written.
 * The call blocks and runs on the handle's stream, all of it enqueued on that one stream; there is no stream-taking form
 * yet.  Device scratch grows with n_bytes, max_frames and (host memory) the decoded size: a batch larger than device
 * memory is the caller's to split, and the call returns FLACENC_HIP_ERR_DEVICE when scratch cannot be had.  Host results
 * reach their slots through one transfer into pinned staging and the handle's host threads
 * (flacenc_hip_set_host_threads), not through a transfer per stream.
 * (`streams` is declared const void*: the descriptor is plain data every binding lays out itself.)
 */
struct flacenc_hip_stream_desc {
  uint64_t offset;           /* the stream's frames: bytes [offset, offset + n_bytes) of `bytes` */
  uint64_t n_bytes;
  uint64_t out_offset;       /* its PCM slot: bytes [out_offset, out_offset + out_capacity) of `out` */
  uint64_t out_capacity;
  uint32_t channels;         /* as for flacenc_hip_decode_pcm */
  uint32_t bits_per_sample;
  uint32_t max_block_size;
  uint32_t bytes_per_sample;
};
typedef struct flacenc_hip_stream_desc flacenc_hip_stream_desc;
int flacenc_hip_decode_streams(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                               size_t n_streams, size_t max_frames, uint8_t* out, uint64_t out_bytes, uint64_t* totals,
                               uint64_t call_totals[2], int memory_kind);

/*
 * MD5 digests (RFC 1321) of a batch of byte spans, one lane of the device per span: span i is bytes [offsets[i],
 * offsets[i] + lengths[i]) of `bytes`, and its 16 digest bytes -- A, B, C, D, each little-endian: what STREAMINFO
 * stores -- go to digests + 16*i.  The call for a host that needs one digest per file of a library: the STREAMINFO MD5 of
 * every stream it encodes (flacenc_hip_encode_pcm leaves the MD5 with the caller) or decodes.
 *   bytes, n_bytes    the buffer the spans lie in; digests: [n_spans][16].  Host (pageable or flacenc_hip_host_alloc) or
 *                     device memory, chosen by memory_kind
 *   offsets, lengths  n_spans entries each, ALWAYS host memory, read before the call returns.  Any byte alignment, any
 *                     length, 0 included (the digest of the empty string).  Spans may overlap, repeat and leave gaps; a
 *                     digest depends on no byte outside its span, and no byte outside a span is read
 * n_spans == 0 is OK.  FLACENC_HIP_ERR_BAD_ARGUMENT: a null pointer, an unknown memory kind, n_spans above 2^24 or a span
 * that reaches past n_bytes (offsets[i] + lengths[i] is checked without overflow); nothing is written then.
 * The call blocks and runs on the handle's stream: one upload of the span table, one launch and, for host memory, one
 * upload of `bytes` and one download of the digests, whatever n_spans is; there is no stream-taking form yet.
 * MD5 is serial inside one span, so the rate comes from the number of spans: on an MI355X 2 048 spans of 320 KiB hash
 * at 185 GB/s, ONE span at under 0.1 GB/s -- an order of magnitude slower than on one host core.  That case is out of
 * scope: a single stream's MD5 stays host work, which is why flacenc_hip_decode_pcm has no MD5 form.
 */
int flacenc_hip_md5_spans(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const uint64_t* offsets,
                          const uint64_t* lengths, size_t n_spans, uint8_t* digests, int memory_kind);
/*
 * flacenc_hip_decode_streams plus the STREAMINFO check's digest of every stream, computed on the device from the PCM
 * before it leaves it.  Bytes in `out`, totals, call_totals, error returns and untouched regions are exactly those of
 * flacenc_hip_decode_streams on the same arguments.  In addition
 *   digests           [n_streams][16], where totals live (memory_kind): digests[s] is the MD5 of the first
 *                     totals[s][1]*channels*bytes_per_sample bytes of stream s's slot -- exactly the bytes the call
 *                     wrote.  For bytes_per_sample == ceil(bits_per_sample / 8) that is the STREAMINFO digest of the
 *                     decoded prefix: of the whole stream when totals[s][3] is 0
 * A stream that stopped early (NO_ROOM, CHAIN, a frame's status) is digested over what was written; a stream of zero
 * samples, and every stream of a call that ends with FLACENC_HIP_INDEX_ERROR, gets the digest of the empty string
 * (d41d8cd98f00b204e9800998ecf8427e).  A null `digests` is FLACENC_HIP_ERR_BAD_ARGUMENT; in every error case nothing is
 * written.  The digests cost at most two more launches and one more transfer than flacenc_hip_decode_streams and no
 * further synchronisation, whatever n_streams is.  No stream-taking form yet.
 */
int flacenc_hip_decode_streams_md5(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                                   size_t n_streams, size_t max_frames, uint8_t* out, uint64_t out_bytes,
                                   uint64_t* totals, uint64_t call_totals[2], int memory_kind, uint8_t* digests);

/*
 * Decoding through errors (what `flac -F` does for one file): flacenc_hip_decode_streams stops a stream at the first
 * byte where no verified frame starts; this call resynchronises on the next verified frame, places every frame where
 * its header says it belongs and puts silence where samples are lost.  bytes, n_bytes, streams, n_streams, max_frames,
 * out, out_bytes and memory_kind, the argument checks, "nothing is written on error" and FLACENC_HIP_INDEX_ERROR (set in
 * call_totals[0], nothing written, all totals zero) are exactly those of flacenc_hip_decode_streams.
 *   origins       host memory, n_streams entries, or NULL for all zeros: the absolute inter-channel sample number that
 *                 byte 0 of the stream's slot stands for (0 for a whole file, a seek point's sample number for a span
 *                 that starts there)
 *   totals        [n_streams][8], where `out` lives; gaps: [max_gaps][3], where `out` lives, may be NULL (then max_gaps
 *                 must be 0); call_totals: [4], host memory
 * The rule, every step a function of the span's bytes, the descriptor and the origin only:
 * 1. The verified candidates of a stream are the byte positions of its span where a header valid for the stream's
 *    channels and bits_per_sample starts whose CRC-8 matches, whose subframes all parse, whose frame lies wholly inside
 *    the span and whose CRC-16 matches.
 * 2. The resynchronising chain: its first frame is the verified candidate at the lowest position of the span; the frame
 *    after frame i is the verified candidate at the lowest position at or behind end(i) = pos(i) + len(i).  (A header
 *    planted inside a chain frame is therefore never a frame.)  A break is every place where the next chain frame does
 *    not start exactly where the one before ended, the bytes in front of the first chain frame and the bytes behind
 *    the last one up to the span's end included.
 * 3. Coded position: P(k) = number(k) * max_block_size under a fixed-blocking header (the descriptor's max_block_size:
 *    STREAMINFO's block size of such a stream), P(k) = number(k) under a variable-blocking header; E(k) = P(k) +
 *    block_size(k).  64-bit arithmetic.
 * 4. Placement: chain frame k is placed when block_size(k) <= max_block_size, P(k) >= origin and P(k) >= the maximum of
 *    E(j) over ALL earlier chain frames j < k, placed or not (the empty maximum is the origin).  Otherwise it is dropped
 *    (a repeated frame, a frame from before the origin, frames in descending order, a block above the maximum).  E does
 *    not decrease over placed frames.
 * 5. Room: with W = channels * bytes_per_sample the placed frames are cut at the first one with (E(k) - origin) * W >
 *    out_capacity: it and every placed frame behind it are not written, and the stop reason is
 *    FLACENC_HIP_DECODE_NO_ROOM.
 * 6. Output: with L = E(last written frame) - origin (0 if none is written) the first L * W bytes of the slot are
 *    defined: sample t of a written frame at slot offset (P - origin + t) * W + c * bytes_per_sample in the
 *    flacenc_hip_pack_le_bytes layout, the value flacenc_hip_decode_streams writes; every byte of [0, L * W) in no
 *    written frame is 0.  Slot bytes from L * W on and bytes of `out` in no slot are untouched.
 * 7. totals[s]: [0] frames written, [1] L, [2] samples of silence inside [0, L), [3] chain frames dropped by 4,
 *    [4] bytes of the span in no chain frame, [5] breaks, [6] the stop reason (0 or NO_ROOM), [7] 0.  A span of 0 bytes
 *    gives all zeros, a span without a verified candidate [4] = n_bytes, [5] = 1 and the rest 0.
 * 8. gaps: every maximal run of silence inside [0, L) of every stream is a record {stream, first_sample, n_samples},
 *    first_sample relative to the slot; ordered by stream index, then position.  The first min(total, max_gaps) records
 *    are written and nothing beyond them; call_totals[2] is the total, so a caller can come back with a larger table.
 * 9. call_totals: [0] frames written over all streams (FLACENC_HIP_INDEX_ERROR in its top bit), [1] the sum of L,
 *    [2] gaps, [3] frames dropped.
 * Consequence: for a stream on which flacenc_hip_decode_streams ends with stop reason 0 and whose frames are numbered
 * consecutively from origin / max_block_size (fixed blocking) or origin (variable blocking), the slot bytes, [0] and [1]
 * are that call's, and [2..6] are 0.  Garbage gives counts, never a fault; no byte outside a span is read as a frame and
 * damage in one stream changes nothing for any other.  Errors: those of flacenc_hip_decode_streams, and
 * FLACENC_HIP_ERR_BAD_ARGUMENT for a NULL gaps with max_gaps > 0.  Launches, synchronisations and transfers do not
 * depend on n_streams or on the damage.  The call blocks and runs on the handle's stream.
 */
int flacenc_hip_recover_streams(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                                size_t n_streams, const uint64_t* origins, size_t max_frames, uint8_t* out,
                                uint64_t out_bytes, uint64_t* totals /* [n_streams][8] */,
                                uint64_t* gaps /* [max_gaps][3], may be NULL */, size_t max_gaps, uint64_t call_totals[4],
                                int memory_kind);

/*
 * Seeking: samples [first_sample, first_sample + n_samples) of streams of a batch, for any number of ranges, in one call
 * -- the crops a model is fed, the seconds a player previews -- without decoding, storing or moving the rest.  Only the
 * frames a range touches are decoded, each only up to the last sample wanted, and only the wanted samples are written.
 *   bytes, n_bytes, streams, n_streams, max_frames, memory_kind   as for flacenc_hip_decode_streams; the call ignores the
 *                    descriptors' out_offset and out_capacity, so one table serves both calls.  A span starts at a frame
 *                    boundary: the stream's first frame or a seek point (a frame's byte offset from a SEEKTABLE or from
 *                    an earlier call).  "Position" counts inter-channel samples from the first sample of the span's first
 *                    frame; a caller that starts a span at a seek point subtracts the seek point's sample number itself
 *   ranges           n_ranges descriptors (struct flacenc_hip_range_desc, 32 bytes each), ALWAYS host memory, read before
 *                    the call returns.  In any order; they may repeat and overlap, and any number may name one stream
 *   out, out_bytes   range r owns the slot [out_offset, out_offset + n_samples*channels*bytes_per_sample) with its
 *                    stream's channels and bytes_per_sample, at any byte offset.  Slots must be disjoint; the library does
 *                    NOT check that (overlapping slots give unspecified bytes in the overlap, never a fault)
 *   totals           [n_ranges][4], where `out` lives
 *   call_totals      host memory in both kinds: [0] the frame decodes run, summed over ranges (a frame two ranges touch
 *                    counts twice), [1] the samples written
 * With P, S and W the PCM, totals[s][1] and totals[s][3] flacenc_hip_decode_streams gives for the range's stream with
 * unlimited room: the range gets samples [first_sample, min(first_sample + n_samples, S)) of P at the start of its slot,
 * byte for byte, and nothing else of `out` is written.  totals[r][0] is the number of samples written.  totals[r][1] is
 * why it stopped: 0 when all n_samples were written, else W when W is non-zero (FLACENC_HIP_DECODE_CHAIN or a frame's
 * status bits), else FLACENC_HIP_DECODE_RANGE_END: the span's chain ended exactly at the span's end, before the range
 * did.  totals[r][2] and [3] are a seek point: the byte offset, from the span's start, of the chain frame that holds
 * first_sample, and that frame's position; when first_sample >= S, where the chain stopped (totals[s][2] and S).  A
 * caller may cache them: offset + totals[r][2] as a later span and first_sample - totals[r][3] as a later range give
 * the same bytes.
 * max_frames bounds the chain frames of all streams together and, separately, the frame decodes of all ranges together.
 * FLACENC_HIP_INDEX_ERROR is set in call_totals[0] under the rules of flacenc_hip_decode_streams, or when the ranges
 * touch more frames than max_frames: then nothing is written, all totals are zero and the caller retries with a larger
 * max_frames.
 * n_ranges == 0 is OK.  Errors are those of flacenc_hip_decode_streams (without the checks of the streams' slots), plus
 * FLACENC_HIP_ERR_BAD_ARGUMENT for a range whose stream >= n_streams, reserved != 0, n_ranges above 2^24, a slot that
 * reaches past out_bytes, or first_sample + n_samples overflowing.  In every error case nothing is written.  Garbage
 * gives a stop reason, never a fault, and changes nothing for ranges on other streams.
 * The call blocks and runs on the handle's stream; its launches, synchronisations and transfers depend on the channel
 * counts the ranges' streams have and on max_frames, not on n_streams or n_ranges.  There is no stream-taking form yet.
 * The same ranges as planar int32 / float32 rows, a [B, C, T] tensor in place: flacenc_hip_decode_ranges_planar below.
 */
#define FLACENC_HIP_DECODE_RANGE_END 1024u
struct flacenc_hip_range_desc {
  uint64_t first_sample;     /* position of the range's first sample in its stream's span */
  uint64_t n_samples;        /* inter-channel samples wanted; 0 is legal */
  uint64_t out_offset;       /* the range's slot: n_samples*channels*bytes_per_sample bytes of `out` from here */
  uint32_t stream;           /* index into `streams` */
  uint32_t reserved;         /* 0 */
};
typedef struct flacenc_hip_range_desc flacenc_hip_range_desc;
int flacenc_hip_decode_ranges(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                              size_t n_streams, const void* ranges, size_t n_ranges, size_t max_frames, uint8_t* out,
                              uint64_t out_bytes, uint64_t* totals, uint64_t call_totals[2], int memory_kind);

/*
 * flacenc_hip_decode_ranges with the output a model reads: every range's samples as planar 4-byte elements, so that a
 * batch of crops is a [B, C, T] int32 or float32 tensor when the call returns, with no pass over the data behind it.
 * bytes, n_bytes, streams, n_streams, ranges, n_ranges, max_frames, totals, call_totals and memory_kind are those of
 * flacenc_hip_decode_ranges -- one pair of tables serves both calls -- and so are totals[r][0..3], call_totals, the
 * FLACENC_HIP_INDEX_ERROR rule (nothing is written, all totals are zero), every error return, "nothing is written on
 * error" and the behaviour on garbage (a stop reason, never a fault, nothing changes for ranges on other streams).  A
 * stream's bytes_per_sample is validated as before and otherwise plays no part in the layout.  What differs is the slot:
 *   out, out_bytes   range r on a stream of C channels owns C * n_samples * 4 bytes from out_offset, a multiple of 4:
 *                    C rows of n_samples elements, element (channel c, sample i) the 4-byte value at out_offset +
 *                    (c * n_samples + i) * 4.  With w = totals[r][0], elements i < w of every row are the decoded
 *                    samples first_sample + i; elements w <= i < n_samples are zero (0, resp. +0.0f).  When the call
 *                    returns FLACENC_HIP_OK without FLACENC_HIP_INDEX_ERROR the whole of every slot is defined; bytes of
 *                    `out` in no slot are untouched.  Slots must be disjoint, unchecked as for flacenc_hip_decode_ranges.
 *                    A batch [B, C, T] is n_samples = T and out_offset = b * C * T * 4
 *   sample_format    FLACENC_HIP_SAMPLE_I32 or FLACENC_HIP_SAMPLE_F32
 * The value rule, for every input -- hand-built frames whose predictions wrap included: the value is the int32 the
 * decoder reconstructs, exactly what flacenc_hip_decode_ranges stores when the stream's bytes_per_sample is 4.
 * FLACENC_HIP_SAMPLE_I32 stores it; FLACENC_HIP_SAMPLE_F32 stores that int32 converted to float with round-to-nearest-
 * even, multiplied by 2^-(bits_per_sample - 1).  For every value that fits the stream's bit depth (at most 24 bits) both
 * steps are exact: the element is the rational value / 2^(bits_per_sample - 1), in [-1, 1).
 * Further FLACENC_HIP_ERR_BAD_ARGUMENT cases, nothing written: an out_offset that is not a multiple of 4, a slot of this
 * size that reaches past out_bytes, an unknown sample_format.
 * Host memory: the ranges' elements come back in one transfer into pinned staging, and the handle's host threads place
 * the rows and zero their tails; the number of transfers does not depend on n_ranges.  Device memory: one launch more
 * than flacenc_hip_decode_ranges (the zero pass over all ranges), whatever n_ranges is.  There is no stream-taking form,
 * as for flacenc_hip_decode_ranges.
 */
#define FLACENC_HIP_SAMPLE_I32 0u   /* the decoded value */
#define FLACENC_HIP_SAMPLE_F32 1u   /* (float)value * 2^-(bits_per_sample - 1) */
int flacenc_hip_decode_ranges_planar(flacenc_hip_handle* h, const uint8_t* bytes, uint64_t n_bytes, const void* streams,
                                     size_t n_streams, const void* ranges, size_t n_ranges, size_t max_frames, void* out,
                                     uint64_t out_bytes, uint32_t sample_format, uint64_t* totals,
                                     uint64_t call_totals[2], int memory_kind);

/*
 * The way there in one call: a batch of PCM streams to FLAC frames, what flacenc_hip_encode_pcm does for one stream, for
 * every stream of a table -- a speech corpus, a sample pack, the tracks of an album -- with a number of synchronisations
 * and transfers that does not depend on the number of streams, and a number of launches that depends only on the
 * classes of streams and the distinct lengths of their last blocks (below).
 *   pcm, pcm_bytes   one buffer that holds every stream's packed interleaved little-endian PCM (the layout of
 *                    flacenc_hip_encode_pcm).  Stream s is bytes [offset, offset + total_samples*channels*
 *                    bytes_per_sample) of it.  Spans may touch, leave gaps, overlap or repeat, at any byte alignment; no
 *                    byte outside a span is read
 *   streams          n_streams descriptors (struct flacenc_hip_pcm_stream_desc, 48 bytes each), ALWAYS host memory,
 *                    read before the call returns
 *   block_size       of every frame but a stream's last, 64..32767 as for flacenc_hip_encode_pcm
 *   out, out_bytes   one buffer for every stream's frames: stream s owns the slot [out_offset, out_offset +
 *                    out_capacity).  Slots must be disjoint; the library does NOT check that (overlapping slots give
 *                    unspecified bytes in the overlap, never a fault)
 *   frame_lengths    max_frames entries of room, at least flacenc_hip_encode_streams_frames(streams, n_streams,
 *                    block_size) = the sum of ceil(total_samples / block_size): the byte length of every frame, stream
 *                    after stream in table order
 *   totals           [n_streams][4]: [0] frames written to the slot, [1] bytes written, [2] the index of the stream's
 *                    first entry in frame_lengths, [3] 0 or FLACENC_HIP_ENCODE_NO_ROOM
 *   call_totals      host memory in both kinds: [0] frames and [1] bytes written over all streams
 *   memory_kind      FLACENC_HIP_MEM_HOST (pageable or flacenc_hip_host_alloc memory) or FLACENC_HIP_MEM_DEVICE: where
 *                    pcm, out, frame_lengths and totals live
 * Per-stream equivalence: for every stream s its slot and frame_lengths[totals[s][2] ..] hold exactly what
 * flacenc_hip_encode_pcm gives for that stream alone on the same handle with the same cfg (flags included), the stream's
 * channels, bytes_per_sample, bits_per_sample and sample_rate, block_size, first_frame_number = 0 and frame_number_step
 * = 1.  Every frame has block_size samples except a stream's last; a last block below 64 samples is the usual Constant /
 * Verbatim frame.  channels == 2 takes the stereo decision, any other count Independent(channels).  Every
 * FLACENC_HIP_FLAG_* the frame-level calls honour is honoured: the same frame-level calls run underneath
 * (flacenc_hip_encode_pack_stereo_frames_async resp. flacenc_hip_encode_pack_frames_async, every frame packed with
 * number 0 and renumbered when it is placed).
 * The one difference: flacenc_hip_encode_pcm returns FLACENC_HIP_ERR_BAD_ARGUMENT when out_capacity is too small; here a
 * slot that is too small gets the longest prefix of whole frames that fits and totals[s][3] = FLACENC_HIP_ENCODE_NO_ROOM;
 * the lengths of the frames behind the cut are still written to frame_lengths.  Slot bytes beyond totals[s][1] and
 * bytes of `out` in no slot are untouched.  n_streams == 0 and streams of 0 samples are OK (no frame, all-zero totals
 * but [2]).
 * FLACENC_HIP_ERR_BAD_ARGUMENT, with nothing written: a null pointer, an unknown memory kind, n_streams above 2^24, a span
 * that reaches past pcm_bytes, a slot that reaches past out_bytes, max_frames below
 * flacenc_hip_encode_streams_frames(...), a stream -- or a call -- of 2^31 frames or more, block_size outside 64..32767,
 * channels outside 1..8, bytes_per_sample outside 1..4, bits_per_sample outside 8..24 -- after
 * flacenc_hip_set_max_encode_bits_per_sample(h, 32) outside 8..32, and more than 24 bits at bytes_per_sample other than 4
 * (flacenc_hip_encode_streams_planar: with FLACENC_HIP_SAMPLE_F32).  A class of more than 24 bits runs
 * the step of flacenc_hip_encode_pack_frames_wide in place of the frame-level calls; every other class runs as it always has.
 * The plan: a class is (channels, bits_per_sample, bytes_per_sample, sample_rate).  The full blocks of all streams of a
 * class are one run, cut into frame-level calls of at most clamp(48 MiB / frame bytes, 768, 8192) frames; the last blocks
 * of a class are one further run PER DISTINCT LENGTH, since the analysis kernels take one block size per launch (a corpus
 * with k distinct tail lengths in a class pays k tail runs).  The call blocks and runs on the handle's stream, all of it
 * enqueued on that one stream (no overlap of transfers with compute, unlike flacenc_hip_encode_pcm: a single long stream is
 * that call's case); there is no stream-taking form yet.  Device scratch grows with the batch (the rows of the largest
 * class, a pack slot per frame, and for host memory the PCM and the frames): a batch larger than device memory is the
 * caller's to split, and the call returns FLACENC_HIP_ERR_DEVICE when scratch cannot be had.  Host results reach their
 * slots through one transfer into pinned staging and the handle's host threads (flacenc_hip_set_host_threads).
 * (`streams` is declared const void*: the descriptor is plain data every binding lays out itself.)
 */
#define FLACENC_HIP_ENCODE_NO_ROOM 256u
struct flacenc_hip_pcm_stream_desc {
  uint64_t offset;           /* the stream's PCM: bytes [offset, offset + total_samples*channels*bytes_per_sample) of `pcm` */
  uint64_t total_samples;    /* inter-channel samples; 0 is legal */
  uint64_t out_offset;       /* its slot: bytes [out_offset, out_offset + out_capacity) of `out` */
  uint64_t out_capacity;
  uint32_t channels;         /* 1..8; 2 = the stereo decision, else Independent(channels), as flacenc_hip_encode_pcm */
  uint32_t bits_per_sample;  /* 8..24; ..32 after flacenc_hip_set_max_encode_bits_per_sample(h, 32) */
  uint32_t bytes_per_sample; /* 1..4 */
  uint32_t sample_rate;
};
typedef struct flacenc_hip_pcm_stream_desc flacenc_hip_pcm_stream_desc;
size_t flacenc_hip_encode_streams_frames(const void* streams, size_t n_streams, uint32_t block_size);
int flacenc_hip_encode_streams(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const uint8_t* pcm,
                               uint64_t pcm_bytes, const void* streams, size_t n_streams, uint32_t block_size,
                               uint8_t* out, uint64_t out_bytes, uint32_t* frame_lengths, size_t max_frames,
                               uint64_t* totals, uint64_t call_totals[2], int memory_kind);

/*
 * The same call on a tensor: planar rows of 4-byte elements in place of packed PCM -- a [B, C, T] int32 or float32
 * tensor as it lies, the slots flacenc_hip_decode_ranges_planar writes -- with the digests of the PCM the frames stand
 * for.  No scale, round, clamp, convert or interleave pass runs in front of the encoder and no packed image of the
 * samples exists anywhere (but where digests are asked for: one, in handle scratch, written once and hashed once).
 * `streams`, out, out_bytes, frame_lengths, max_frames, totals, call_totals, memory_kind and
 * flacenc_hip_encode_streams_frames are flacenc_hip_encode_streams's; one table serves both calls.
 *   samples, samples_bytes, row_pitch
 *                    stream s is `channels` rows: row c starts at byte offset + c * pitch * 4 of `samples` (offset a
 *                    multiple of 4; device memory: `samples` 4-byte aligned), its elements [0, total_samples) are its
 *                    samples.  pitch is row_pitch where that is non-zero (it must then be at least every stream's
 *                    total_samples) and the stream's own total_samples where it is 0 (tight rows).  A [B, C, T] tensor
 *                    with a length per item: row_pitch = T, offset = b*C*T*4, total_samples = length[b].  Streams may
 *                    share, overlap or repeat rows.  No element outside the valid elements of a stream's rows has any
 *                    influence on any output; on the device none is read (host memory: the bytes between the first and
 *                    the last valid element go to the device in one transfer)
 *   sample_format    FLACENC_HIP_SAMPLE_I32: the element is the sample.  FLACENC_HIP_SAMPLE_F32: the sample is
 *                    q(x) = clamp(rne(x * 2^(bits_per_sample-1)), -2^(bits_per_sample-1), 2^(bits_per_sample-1) - 1),
 *                    the product formed in float32 (exact short of overflow), rne round-to-nearest-even, +-inf clamped,
 *                    every NaN 0: the inverse of the decoder's FLACENC_HIP_SAMPLE_F32 rule, q((float)v * 2^-(bits-1)) == v
 *                    for every v of the depth
 *   bytes_per_sample (of the descriptor) is checked as in flacenc_hip_encode_streams and plays no part in reading
 *                    `samples`: it is the sample width of the packed PCM P_s the rules below are stated over
 *   digests          NULL, or [n_streams][16] where totals lives: the MD5 of all of P_s, whether or not the slot had
 *                    room for every frame -- the STREAMINFO digest when bytes_per_sample == ceil(bits_per_sample/8); a
 *                    stream of 0 samples gets the digest of the empty string
 *   clipped          NULL, or [n_streams] where totals lives: F32: the elements, over all channels, where q clamped or
 *                    met a NaN; I32: 0
 * Equivalence: let P_s be the packed interleaved little-endian PCM, bytes_per_sample bytes a sample, of stream s's
 * samples.  out, frame_lengths, totals, call_totals, the FLACENC_HIP_ENCODE_NO_ROOM rule, what stays untouched and every
 * error return are byte for byte what flacenc_hip_encode_streams gives on a buffer holding the P_s with the same table,
 * cfg, flags, block_size and slots.  I32 elements that do not fit bits_per_sample: as flacenc_hip_encode_streams on those
 * int32 values stored at bytes_per_sample = 4 (P_s, and so the digest, keeps their low bytes_per_sample bytes).
 * FLACENC_HIP_ERR_BAD_ARGUMENT, with nothing written, also for: an offset that is no multiple of 4, an unknown
 * sample_format, a non-zero row_pitch below some stream's total_samples, rows that reach past samples_bytes.
 * Cost: the synchronisations, transfers and launches of flacenc_hip_encode_streams for the same table (this call's fill
 * in place of that call's), plus two launches where digests are asked for (one where the table holds no frame); digests
 * and clip counts come down in the result transfer that is there anyway.
 */
int flacenc_hip_encode_streams_planar(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const void* samples,
                                      uint64_t samples_bytes, uint32_t sample_format, uint64_t row_pitch,
                                      const void* streams, size_t n_streams, uint32_t block_size, uint8_t* out,
                                      uint64_t out_bytes, uint32_t* frame_lengths, size_t max_frames, uint64_t* totals,
                                      uint64_t call_totals[2], uint8_t* digests, uint64_t* clipped, int memory_kind);

/* ---- block-size search: variable-blocking streams ------------------------------------------------------------ */
/*
 * Each region coded at the block size that compresses it best (BASELINE config 5's "beat-search block sizing"; the
 * reference snapshot has no such mode, so this is an extension like FLACENC_HIP_FLAG_ALLOW_ORDER_32).  The input is cut
 * into superblocks of block_size = S samples; a full superblock may be coded as any binary tiling into blocks of S, S/2,
 * .., S/2^(levels-1).  Nodes are numbered in heap order (node 1 the superblock, children of n are 2n and 2n+1); node n
 * costs the exact byte length of its block coded as a variable-blocking frame, and bottom-up node n is split exactly when
 * its children's best sum is strictly smaller (ties keep the larger block).  A last partial superblock of
 * total_samples % S samples is one frame, never split.
 * Every chosen frame's bytes between header and CRC-16 are exactly what the fixed-blocking encode+pack call
 * (flacenc_hip_encode_pack_stereo_frames_async for 2 channels, flacenc_hip_encode_pack_frames_async otherwise) writes for
 * those samples at that block size under the same config and flags; its header uses variable blocking (sync 0xFFF9, the
 * coded number = first_sample_number + the block's first sample offset, up to 36 bits), with both CRCs recomputed.
 *   frames        FrameBuf layout at S: channel c of superblock i at frames + (i*channels + c)*stride, zero beyond
 *                 total_samples (what flacenc_hip_fill_le_bytes writes)
 *   levels        1..5; S must be divisible by 2^(levels-1) with S / 2^(levels-1) >= 256 (levels 1: S >= 256)
 *   out           the chosen frames back to back (out_capacity bytes of room); per output frame its byte offset in out,
 *                 length and block size (max_frames entries of room); split_masks (NULL to skip): per superblock bit
 *                 n - 1 set for every split node n of its chosen tiling; totals[0] = frames, totals[1] = bytes
 * When the frames or bytes exceed max_frames / out_capacity, nothing is written to out or the per-frame arrays, totals[0]
 * carries FLACENC_HIP_VARIABLE_OVERFLOW and totals hold what a call with enough room needs.  first_sample_number +
 * total_samples must not exceed 2^36.  flacenc_hip_variable_bytes_bound / _max_frames give room that always suffices
 * (0 for arguments the encoder rejects).  The async form takes device pointers and enqueues everything on `stream` in the
 * handle's scratch; flacenc_hip_encode_variable takes host or device pointers and returns when the outputs are there.
 */
#define FLACENC_HIP_VARIABLE_OVERFLOW 0x8000000000000000ull
size_t flacenc_hip_variable_bytes_bound(uint32_t channels, uint32_t block_size, uint32_t levels,
                                        uint32_t bits_per_sample, uint64_t total_samples);
size_t flacenc_hip_variable_max_frames(uint32_t block_size, uint32_t levels, uint64_t total_samples);
int flacenc_hip_encode_variable_async(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                                      uint64_t total_samples, uint32_t channels, uint32_t block_size, uint32_t levels,
                                      size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                      uint64_t first_sample_number, uint8_t* out, size_t out_capacity,
                                      uint64_t* frame_offsets, uint32_t* frame_lengths, uint32_t* frame_block_sizes,
                                      size_t max_frames, uint32_t* split_masks, uint64_t* totals, void* stream);
int flacenc_hip_encode_variable(flacenc_hip_handle* h, const flacenc_hip_frame_config* cfg, const int32_t* frames,
                                uint64_t total_samples, uint32_t channels, uint32_t block_size, uint32_t levels,
                                size_t stride, uint32_t bits_per_sample, uint32_t sample_rate,
                                uint64_t first_sample_number, uint8_t* out, size_t out_capacity, uint64_t* frame_offsets,
                                uint32_t* frame_lengths, uint32_t* frame_block_sizes, size_t max_frames,
                                uint32_t* split_masks, uint64_t* totals, int memory_kind);

int flacenc_hip_synchronize(flacenc_hip_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* FLACENC_HIP_H_ */
