/*
 * lut_ldpc_hip.h -- C-ABI of the MI355X LUT-LDPC decode path (liblut_ldpc_amd.so).
 *
 * This is the drop-in boundary for the hot path of mmeidlinger/lut_ldpc.  The reference has
 * no FFI layer: the seam is the C++ virtual call `C->decode(softbits)` made once per frame by
 * LDPC_BER_Sim::sim_snr_point (src/LDPC_BER_Sim.cpp:281), landing in
 * LDPC_Code_LUT::decode / lut_decode (src/LDPC_Code_LUT.cpp:204,259).  The entry points below
 * are what an LDPC_Code_LUT-shaped class binds instead (see INTEGRATION.md for the stub);
 * the class shipped in lut_ldpc_amd/csrc/host does exactly that.
 *
 * Conventions: plain pointers and sizes, int return codes (0 = ok, <0 = error, text via
 * lutldpc_last_error()), no exceptions cross the boundary.  A decoder handle owns its device
 * memory and one HIP stream and is NOT re-entrant (like the reference object, whose
 * lut_decode mutates the member `msgs`, src/LDPC_Code_LUT.hpp:311): use one handle per host
 * thread.  All label arrays are uint8 and frame-major: element [f*nvar + v].
 *
 * Errors of the batch entries (every entry below that takes a batch size B): argument errors before state errors.  A NULL
 * handle or B <= 0 is LUTLDPC_ERR_ARG on any handle; a handle created without a device (device < 0, host-only) then answers
 * LUTLDPC_ERR_STATE, with one message text for all entries; only then is the handle's device made current.  The checks an
 * entry documents for its own arguments keep the places given with it.
 */
#ifndef LUT_LDPC_HIP_H
#define LUT_LDPC_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUTLDPC_OK               0
#define LUTLDPC_ERR_ARG         -1   /* bad argument / inconsistent sizes                */
#define LUTLDPC_ERR_PARSE       -2   /* malformed tree text                               */
#define LUTLDPC_ERR_UNSUPPORTED -3   /* e.g. node fan-in or table beyond device limits    */
#define LUTLDPC_ERR_HIP         -4   /* HIP runtime failure (no device, OOM, launch)      */
#define LUTLDPC_ERR_STATE       -5   /* call order (e.g. decode before set-up)            */

typedef struct lutldpc_decoder lutldpc_decoder;

/* Text of the last error on the calling thread ("" if none). */
const char *lutldpc_last_error(void);

/* Library / build identification, e.g. "lut_ldpc_amd 0.1 gfx950". */
const char *lutldpc_version(void);

/* Number of visible HIP devices (0 without a GPU; never fails). */
int lutldpc_device_count(void);

/*
 * Create a decoder.  Replaces the state built by LDPC_Code_LUT::set_code ->
 * decoder_parameterization (src/LDPC_Code_LUT.cpp:471-541) and set_trees (:120-169).
 *
 *   nvar, nchk      code dimensions
 *   dv[nvar]        variable-node degrees   (reference member dv_vec)
 *   dc[nchk]        check-node degrees      (reference member dc_vec)
 *   cn_msg_idx[E]   for each check, in order, the VN-major edge ids of its edges
 *                   (reference member cn_msg_idx, :507-527); E = sum(dv) = sum(dc)
 *   Nq_Cha          channel alphabet size
 *   Nq_Msg[max_iters], reuse_vec[max_iters]   message alphabets / LUT reuse pattern
 *   min_lut         1: min-sum check update (chk_update_minsum, :355), 0: CHKTREE LUTs
 *   var_trees_txt   Array<Array<LUT_Tree>> in the reference's own text serialisation
 *                   (src/LUT_Tree.cpp:847-865, the `var_tree_string` of lut_codec.it,
 *                   src/LDPC_Code_LUT.cpp:677-678): [tree set][degree class]
 *   chk_trees_txt   same for check trees; NULL or "" when min_lut
 *   device          HIP device ordinal
 * The exit conditions default to the reference constructor's (max_iters, psc=1, pisc=0).
 */
int lutldpc_decoder_create(int nvar, int nchk, const int32_t *dv, const int32_t *dc,
                           const int32_t *cn_msg_idx,
                           int Nq_Cha, const int32_t *Nq_Msg, const uint8_t *reuse_vec, int max_iters,
                           int min_lut, const char *var_trees_txt, const char *chk_trees_txt,
                           int device, lutldpc_decoder **out);

int lutldpc_decoder_destroy(lutldpc_decoder *d);

/* LDPC_Code_LUT::set_exit_conditions (src/LDPC_Code_LUT.cpp:176-185).  max_iters must not
 * exceed the value given at creation (the tree sets are indexed by iteration). */
int lutldpc_decoder_set_exit_conditions(lutldpc_decoder *d, int max_iters, int psc, int pisc);

/*
 * Batched LDPC_Code_LUT::lut_decode (src/LDPC_Code_LUT.cpp:259-353) on host buffers.
 *   cha[B*nvar]       quantised channel labels   (LLRin_cha)
 *   msg0[B*nvar]      initial message labels     (LLRin_msg)
 *   out_bits[B*nvar]  decoded bits 0/1           (LLRout)
 *   out_iters[B]      the reference's return value per frame: 0, ii+1, +max_iters or -max_iters
 * Frames are independent; results are bit-identical to calling lut_decode frame by frame.
 * Errors instead of the reference's it_assert aborts: B <= 0 or a null pointer -> LUTLDPC_ERR_ARG; a handle without a device
 * -> LUTLDPC_ERR_STATE.  A label outside its alphabet (>= Nq_Cha, >= Nq_Msg[0]) is undefined behaviour in the reference (it
 * indexes the tables unchecked); here it is clamped to the largest label when the rows are built, so it can never reach
 * another frame's lane.
 */
int lutldpc_decoder_decode_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B,
                                 uint8_t *out_bits, int32_t *out_iters);

/*
 * lutldpc_decoder_decode_batch for callers whose labels cross a host link: the same decode, bit for bit, without the bytes that
 * carry no information.  Labels may come two per byte, the initial messages may be derived from the channel labels on the device
 * (the toolkit's QCHA mode, cha2msg_map of src/LDPC_Code_LUT.cpp:204-226), and only a window of the decided bits is returned, one
 * bit each -- the data bits are the first nvar - rank(H).
 *   cha        host [B][stride] labels in `in_format`: stride = nvar (LUTLDPC_IN_BYTES) or ceil(nvar/2) (LUTLDPC_IN_NIBBLES)
 *   msg0       the initial message labels in the same format, or NULL when io->cha2msg_map is given
 *   out_words  host [B][ceil(out_count/32)] uint32: bit j of word w = decided bit out_first + 32w + j, bits beyond out_count are 0;
 *              NULL when only the iteration codes are wanted
 *   out_iters  host [B] as lutldpc_decoder_decode_batch; may be NULL
 * A channel label >= Nq_Cha is clamped to the largest label (a 6-label alphabet in a nibble can hold one), the map is applied after
 * the clamp; a given msg0 is clamped to Nq_Msg[0] - 1.
 * Errors: NULL handle or B <= 0 -> LUTLDPC_ERR_ARG; then the entry's own arguments, LUTLDPC_ERR_ARG too: NULL io or cha, an
 * in_format other than the two below, LUTLDPC_IN_NIBBLES with Nq_Cha > 16 (or with Nq_Msg[0] > 16 and msg0 given), both or neither
 * of msg0 and cha2msg_map, a map entry outside [0, Nq_Msg[0]), out_first < 0, out_count < 1, out_first + out_count > nvar; only
 * then a handle without a device -> LUTLDPC_ERR_STATE.
 */
#define LUTLDPC_IN_BYTES   0   /* one label per byte, [B][nvar], as decode_batch                                   */
#define LUTLDPC_IN_NIBBLES 1   /* two labels per byte, frame stride ceil(nvar/2) bytes, node v in byte v/2,
                                  even v in bits 0-3, odd v in bits 4-7; the spare nibble of an odd nvar is ignored */
typedef struct {
    int32_t in_format;            /* applies to cha and, when given, to msg0                                  */
    const int32_t *cha2msg_map;   /* NULL: msg0 is given.  Else Nq_Cha entries < Nq_Msg[0]: msg0[v] = map[cha[v]]
                                     computed on the device, msg0 must be NULL                                 */
    int32_t out_first, out_count; /* decided bits out_first .. out_first+out_count-1 of every frame            */
} lutldpc_packed_io;

int lutldpc_decoder_decode_batch_packed(lutldpc_decoder *d, const lutldpc_packed_io *io, const uint8_t *cha, const uint8_t *msg0,
                                        int B, uint32_t *out_words, int32_t *out_iters);

/* Same with device-resident buffers (same frame-major layout); asynchronous on the decoder's
 * stream unless `sync` is non-zero.  The call runs on the decoder's OWN non-blocking stream (lutldpc_decoder_stream): the input
 * buffers must be complete, and the four buffers must not be memory that another stream is still working on (a stream-ordered
 * allocator may hand out a block whose last users have not finished on THEIR stream) -- synchronise, or make the decoder's
 * stream wait on an event, before the call.  The inputs are read for the whole duration of the decode (the LDS-resident
 * decoder reads them in place), the outputs are written by it. */
int lutldpc_decoder_decode_batch_device(lutldpc_decoder *d, const uint8_t *d_cha, const uint8_t *d_msg0, int B,
                                        uint8_t *d_out_bits, int32_t *d_out_iters, int sync);

/* lut_decode of a small batch with the message dumps of LDPC_Code_LUT::set_output_verbosity(level), level 2 or 3
 * (src/LDPC_Code_LUT.cpp:292-298 initial messages, :311-317 after every check update (level 3), :331-337 after every variable
 * update): trace[dump][B][E] label bytes in the reference's print order, *n_dumps = 1 + max_iters * (level - 1).  Debug path
 * (per-class streaming launches, one copy per dump); which dumps the reference would have PRINTED for a frame follows from its
 * iteration code (a frame that leaves through the exit test returns before the dump of its last variable update). */
int lutldpc_decoder_decode_batch_trace(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, int B, int level, uint8_t *out_bits,
                                       int32_t *out_iters, uint8_t *trace, int64_t trace_cap, int32_t *n_dumps);

/*
 * Batched LDPC_Code_LUT::decode(const vec&, bvec&) (src/LDPC_Code_LUT.cpp:204-226):
 * quant_nonlin with the boundaries qb_Cha / qb_Msg (src/common.cpp:120-138), initial
 * messages by mode (0 = CONT: quant_nonlin(llr, qb_Msg); 1 = QCHA: cha2msg_map[label]),
 * then lut_decode.  llr[B*nvar] double, host memory.  out_bits holds all nvar bits per
 * frame; the systematic part is the first nvar - rank(H) of them (:225).
 * The quantiser is the one of lutldpc_decoder_decode_llr_packed below, on float64.  The boundary arrays are taken as the caller
 * holds them, sorted or not: the label is the number of LEADING boundaries below x on ANY array (the loop of quant_nonlin stops at
 * the first boundary that x does not exceed; a NaN boundary stops every x), which the entry turns into the plain count over the
 * running maxima.  Mode 0 ignores a given map; mode 1 ignores qb_Msg and n_qb_Msg, and a cha2msg_map entry outside
 * [0, Nq_Msg[0]) is LUTLDPC_ERR_ARG (no label outside its alphabet reaches the decoder).
 */
int lutldpc_decoder_decode_llr_batch(lutldpc_decoder *d, const double *llr, int B,
                                     const double *qb_Cha, int n_qb_Cha,
                                     const double *qb_Msg, int n_qb_Msg,
                                     int initial_message_mode, const int32_t *cha2msg_map,
                                     uint8_t *out_bits, int32_t *out_iters);

/*
 * lutldpc_decoder_decode_llr_batch for receivers: the same quantiser and decode, bit for bit, for soft values as a demapper
 * holds them -- float64, float32, float16 or int8 with a scale, in host memory or already on the device -- and a window of the
 * decided bits out at one bit each.  The values are quantised straight into both label row sets (no frame-major labels in
 * between), the decode is that of every other batch entry.  Unlike that entry this one refuses boundaries that are not
 * non-decreasing or hold NaN, and a map in mode 0.
 *   llr        [B][frame_stride] elements of io->dtype; host memory (io->on_device = 0) or device memory (1), aligned to its element
 *              size.  Elements nvar .. frame_stride-1 of a frame are never read.
 *   out_words  [B][ceil(out_count/32)] uint32 as lutldpc_decoder_decode_batch_packed, or NULL
 *   out_iters  [B] as lutldpc_decoder_decode_batch, or NULL
 *   out_cha, out_msg0   optional [B][nvar] label bytes: what the device derived from the values
 * Every output lives where llr lives.  With out_words and out_iters both NULL the decode is skipped and the call only quantises;
 * at least one output must be asked for.
 * The value of an element is x as a real number (int8: (double)q * scale); cha = number of leading qb_Cha[k] with x > qb_Cha[k],
 * msg0 = the same over qb_Msg (mode 0, CONT) or cha2msg_map[cha] (mode 1, QCHA): quant_nonlin of src/common.cpp:120-129 on the
 * value, so NaN gets label 0, +inf the largest label and -0.0 is 0.  No value is rounded on the way: the boundaries are rounded
 * DOWN to the input type on the host, which leaves every comparison as it was.
 * on_device = 1: the contract of lutldpc_decoder_decode_batch_device -- the call runs on the decoder's own stream, its buffers must
 * be complete and not in use by another stream, and it is asynchronous unless io->sync is set.  on_device = 0: synchronous.
 * Errors: NULL handle or B <= 0 -> LUTLDPC_ERR_ARG; then the entry's own arguments, LUTLDPC_ERR_ARG too: NULL io or llr, an
 * unknown dtype, llr not aligned to its element size, frame_stride neither 0 nor >= nvar, n_qb_Cha != Nq_Cha - 1 (mode 0:
 * n_qb_Msg != Nq_Msg[0] - 1), a NaN or descending boundary, a mode other than 0 / 1, mode 0 without qb_Msg or with a map, mode 1
 * without a map, a map entry outside [0, Nq_Msg[0]), a window outside [0, nvar) when out_words is given, LUTLDPC_LLR_I8 with a
 * scale that is not finite and positive, no output asked for; only then a handle without a device -> LUTLDPC_ERR_STATE.
 */
#define LUTLDPC_LLR_F64 0
#define LUTLDPC_LLR_F32 1
#define LUTLDPC_LLR_F16 2      /* IEEE binary16 */
#define LUTLDPC_LLR_I8  3      /* LLR = scale * q */
typedef struct {
    int32_t dtype;
    int32_t on_device;           /* 0: llr and every output are host memory; 1: all of them are device memory */
    int64_t frame_stride;        /* elements from one frame to the next; 0 = nvar, else >= nvar */
    double  scale;               /* LUTLDPC_LLR_I8: finite, > 0; ignored otherwise */
    const double *qb_Cha; int32_t n_qb_Cha;          /* host, Nq_Cha - 1 */
    const double *qb_Msg; int32_t n_qb_Msg;          /* host, Nq_Msg[0] - 1; mode 0 only */
    int32_t initial_message_mode; const int32_t *cha2msg_map;   /* host; mode 1 only, entries in [0, Nq_Msg[0]) */
    int32_t out_first, out_count;                    /* window of decided bits, as lutldpc_packed_io */
    int32_t sync;                                    /* on_device = 1: synchronise the decoder's stream before returning */
} lutldpc_llr_io;
int lutldpc_decoder_decode_llr_packed(lutldpc_decoder *d, const lutldpc_llr_io *io, const void *llr, int B,
                                      uint32_t *out_words, int32_t *out_iters, uint8_t *out_cha, uint8_t *out_msg0);

/* The host half of that entry, without a decoder or a device (self test): the thresholds in the input type (widened to double,
 * ascending, at most 255; none for LUTLDPC_LLR_I8, whose byte is its own cell) and the two 256-entry tables from a value's cell
 * = #{j : x > thr[j]} to its labels.  Reads dtype, scale, the boundaries, the mode and the map of io; the same argument errors,
 * and LUTLDPC_ERR_ARG when thr_cap is short. */
int lutldpc_llr_cell_table(const lutldpc_llr_io *io, int Nq_Cha, int Nq_Msg0,
                           double *thr, int32_t thr_cap, int32_t *n_thr,   /* the T values, widened to double */
                           uint8_t lut_cha[256], uint8_t lut_msg[256]);

/*
 * Monte-Carlo front end + decode + error counting for B consecutive frames of one SNR point:
 * the body of the frame loop of LDPC_BER_Sim::sim_snr_point (src/LDPC_BER_Sim.cpp:260-286)
 * without the stop rule, which stays with the caller (it needs the frames in order).
 *
 * The channel is described by the partition of the received value into cells (see
 * lut_ldpc_amd/csrc/hip/kernels_frontend.hpp): n_cells cells with cumulative probabilities
 * thr[j] = floor(2^64 * P(cell <= j | bit 0 sent)) for j < n_cells-1 and, per cell, the channel
 * label, initial message label and slicer sign for a sent 0 and the labels of the mirrored cell
 * for a sent 1.  Frame f of the SNR point uses the Philox4x32-10 stream
 * (key = seed, counter = (f_lo, f_hi, bit-pair index, stream)), so any split of the frame range
 * over calls / GPUs generates the same frames.
 *   stream      0 .. LUTLDPC_STREAM_MAX = 2^31 - 1.  Bit 31 of counter word 3 separates the information-bit stream of the random
 *               codewords (stream | 0x80000000, below) from the channel stream: a stream with that bit set would draw its noise
 *               from the blocks that make another stream's data.  Every entry that takes a stream (sim_batch, sim_batch_random,
 *               sample_labels, encode_random, sim_batch_histogram, sim_batch_events and the lutldpc_codec_* wrappers) answers a
 *               larger one with LUTLDPC_ERR_ARG before anything is computed or written; lutldpc_check_stream is that check.
 *   codewords   host [B*nvar] sent bits, bytes 0 or 1 (as encode_random returns them; bit 0 of a byte is what counts: the
 *               device keeps the sent bits in one form, a bitmap per node and frame group), or NULL for the all-zero codeword
 *   K_info      number of leading bits counted as data bits (nvar - rank(H))
 *   frame_stats host [B*4] int32: {lut_decode return value, frame error 0/1, data bit errors,
 *               uncoded (slicer) bit errors over all nvar bits}
 *   cha_out, bits_out  optional host [B*nvar]: the sampled channel labels and the decided bits
 *               (for the "Stimuli Pair" dump of src/LDPC_Code_LUT.cpp:228-238); NULL to skip
 */
typedef struct {
    int32_t n_cells;
    const uint64_t *thr;        /* n_cells-1 */
    const uint8_t *cha_label;   /* n_cells each */
    const uint8_t *msg_label;
    const uint8_t *slicer_neg;
    const uint8_t *cha_label_mirror;
    const uint8_t *msg_label_mirror;
} lutldpc_channel_cells;

#define LUTLDPC_STREAM_MAX 0x7FFFFFFFu
int lutldpc_check_stream(uint32_t stream);   /* LUTLDPC_OK, or LUTLDPC_ERR_ARG and the reason as the last error */

int lutldpc_decoder_sim_batch(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream,
                              uint64_t frame0, int B, const uint8_t *codewords, int K_info, int32_t *frame_stats,
                              uint8_t *cha_out, uint8_t *bits_out);

/* Random codewords made on the device (LDPC.zero_codeword = false).  The codeword of frame f is a pure function of
 * (seed, stream, f): information bits from Philox4x32-10 with key = seed, counter = (f lo, f hi, k/128, stream | 0x80000000)
 * (bit k = bit k%32 of output word (k%128)/32, as random_info_bits of the host driver), parity bit i = popcount(A_i & u) mod 2
 * over the generator's dense parity rows; codeword = [u | parity] in the decoder's column order.
 *
 * set_generator: rows = R rows of ceil(K/64) words (bit j of word w = information bit 64w + j), K + R = nvar; copied to the
 *   device, replaces an earlier generator.  ERR_ARG: rows NULL or K + R != nvar; ERR_STATE: host-only handle;
 *   ERR_UNSUPPORTED: K > 8192 (the sparse form below has no such limit).  describe() gains "generator": {"K":.., "R":..}.
 * set_sparse_generator: the generator as a sparse triangular system, for codes H = [A | T] with T (a permutation of) a triangular
 *   matrix, of any size: codeword bit K+i = XOR of the codeword bits cols[row_ptr[i] .. row_ptr[i+1]), entries in [0, K+R), any
 *   order; parity bits may name other parity bits as long as no bit depends on itself.  The library finds the solve order
 *   (topological sort) and encodes on bit rows (kernels_encode_sparse.hpp).  Works on any handle with K + R = nvar; the handle's
 *   graph is not looked at.  Either setter replaces an earlier generator of either form; a refused call leaves it in place.
 *   ERR_ARG: a NULL array, K < 1, R < 0, K + R != nvar, row_ptr not ascending from 0, an entry outside [0, K+R), a row that names
 *   its own bit, a dependency cycle (the message names one bit on it); then ERR_STATE: host-only handle.
 *   describe() gains "generator": {"K", "R", "form": "sparse", "terms", "block", "depth"}: the number of terms, the parity bits per
 *   block of the blocked solve, the bits on the longest chain of parity-on-parity dependencies.
 *   Every entry below runs the kernels of the form that was set last.
 * encode_random: the codewords of frames frame0 .. frame0+B-1; codewords = host [B*nvar] bytes (0/1), or NULL to keep
 *   them on the device only.  ERR_STATE without a generator.
 * sim_batch_random: lutldpc_decoder_sim_batch with those codewords as the sent ones (same seed / stream for the info bits
 *   and the channel): no host encoding, no upload.  ERR_STATE without a generator. */
int lutldpc_decoder_set_generator(lutldpc_decoder *d, int K, int R, const uint64_t *rows);
int lutldpc_decoder_set_sparse_generator(lutldpc_decoder *d, int K, int R, const int32_t *row_ptr /* R+1 */, const int32_t *cols);
int lutldpc_decoder_encode_random(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, uint8_t *codewords);
int lutldpc_decoder_sim_batch_random(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream,
                                     uint64_t frame0, int B, int K_info, int32_t *frame_stats, uint8_t *cha_out, uint8_t *bits_out);

/*
 * The caller's data bits encoded on the device: the transmit-side counterpart of lutldpc_decoder_decode_batch_packed /
 * lutldpc_decoder_decode_llr_packed, in the bit-packed format those return.  Codeword = [u | parity] in the decoder's column order,
 * parity bit i = popcount(A_i & u) mod 2 over the rows given to lutldpc_decoder_set_generator (K information bits, R rows).
 *   info       [B][in_stride] uint32: bit j of word w of a frame = information bit 32w + j (the layout of out_words).  Bits at
 *              positions >= K of the last word are ignored; words ceil(K/32) .. in_stride-1 of a frame are never read by the kernel.
 *   out_words  [B][ceil(out_count/32)] uint32: bit j of word w = codeword bit out_first + 32w + j, bits beyond out_count are 0.
 *              (0, nvar) is the whole codeword, (K, R) the parity alone.
 * Both buffers live in host memory (io->on_device = 0; the call is synchronous) or both in device memory (1): then the contract of
 * lutldpc_decoder_decode_batch_device holds -- the call runs on the decoder's own stream, the buffers must be complete and not in
 * use by another stream, and it is asynchronous unless io->sync is set.  Only 4-byte alignment is asked of either pointer.
 * The entry reads the generator only: it needs no label rows, leaves the state of the decode entries alone, and a refused call
 * writes nothing.
 * Errors: NULL handle or B <= 0 -> LUTLDPC_ERR_ARG; then the entry's own arguments, LUTLDPC_ERR_ARG too: NULL io, info or out_words,
 * a pointer not 4-byte aligned, in_stride negative or (where a generator is set, which gives K) positive and below ceil(K/32),
 * out_first < 0, out_count < 1, out_first + out_count > nvar; then a handle without a device -> LUTLDPC_ERR_STATE; then no
 * generator set -> LUTLDPC_ERR_STATE (lutldpc_decoder_set_generator comes first).
 */
typedef struct {
    int32_t on_device;            /* 0: info and out_words are host memory; 1: both are device memory */
    int64_t in_stride;            /* uint32 words from one frame to the next; 0 = ceil(K/32), else >= ceil(K/32) */
    int32_t out_first, out_count; /* codeword bits out_first .. out_first+out_count-1, as lutldpc_packed_io */
    int32_t sync;                 /* on_device = 1: synchronise the decoder's stream before returning */
} lutldpc_encode_io;
int lutldpc_decoder_encode_packed(lutldpc_decoder *d, const lutldpc_encode_io *io, const uint32_t *info, int B, uint32_t *out_words);

/* The labels the sampler would produce for those frames (host, frame-major [B*nvar]); codewords as for sim_batch; for tests. */
int lutldpc_decoder_sample_labels(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream,
                                  uint64_t frame0, int B, const uint8_t *codewords, uint8_t *cha, uint8_t *msg0);

/*
 * Per-node channel classes of the sampler: punctured nodes (an erasure), known nodes (shortening, pilots), code bits of unequal
 * reliability (the same channel at another SNR).  The handle keeps up to LUTLDPC_MAX_NODE_CLASSES cell tables and a class per
 * node; the five entries that take `cells` -- sim_batch, sim_batch_random, sample_labels, sim_batch_histogram, sim_batch_events --
 * sample with them when they are called with cells = NULL:
 *   cells != NULL                      the caller's one table on every node, as ever; the handle's node channels are ignored
 *   cells == NULL, node channels set   node v is sampled with tables[node_class[v]]
 *   cells == NULL, none set            LUTLDPC_ERR_ARG (after the checks that come before the table: a host-only handle still
 *                                      answers LUTLDPC_ERR_STATE)
 * The sampling rule is that of one table, node by node: the 64-bit uniform of (frame, node v) does not depend on the table; the
 * cell is the number of thresholds of tables[node_class[v]] that are <= it; labels, mirrored labels for a sent 1 and slicer_neg
 * into frame_stats[3] as with one table.  The stop rule, K_info and the other columns of frame_stats are untouched: a caller who
 * punctures accounts for the effective rate.
 * set_node_channels: every table is checked as the `cells` of sim_batch (NULL member, n_cells 1..72, ascending thresholds, labels
 *   inside the alphabets), every node_class[v] < n_classes: LUTLDPC_ERR_ARG; then a host-only handle: LUTLDPC_ERR_STATE.  The
 *   tables, their bucket indices and the class bytes are copied to the device, into buffers the handle allocates once: setting
 *   new tables per SNR point or per batch costs two small copies.  A call refused with LUTLDPC_ERR_ARG or LUTLDPC_ERR_STATE leaves
 *   the earlier setting in place; after a LUTLDPC_ERR_HIP no classes are set.
 *   n_classes = 0 or nc = NULL clears.  Clearing is a call like any other: on a host-only handle, which can never hold classes, it
 *   too answers LUTLDPC_ERR_STATE (nothing was set, nothing changes) -- a caller that clears unconditionally may ignore that code.  describe() shows "node_channels": {"classes": n, "nodes": [nodes of every class]} while set.
 *   The limit of 16 is what the sampler keeps in LDS: 16 * (576 + 288 + 1024) bytes.
 */
#define LUTLDPC_MAX_NODE_CLASSES 16
typedef struct {
    int32_t n_classes;                     /* 1 .. LUTLDPC_MAX_NODE_CLASSES; 0 clears */
    const lutldpc_channel_cells *tables;   /* n_classes tables, each as sim_batch takes one */
    const uint8_t *node_class;             /* nvar entries < n_classes; a class may have no node */
} lutldpc_node_channels;
int lutldpc_decoder_set_node_channels(lutldpc_decoder *d, const lutldpc_node_channels *nc);

/*
 * Message-label histograms per dump, counted on the device (lut_ldpc_amd/csrc/hip/kernels_stats.hpp): the distribution of the
 * edge-message labels of a finite-length decode, to hold against the densities the LUT design assumed.
 *
 * Dumps are those of set_output_verbosity(level), in the order and number of lutldpc_decoder_decode_batch_trace:
 * n_dumps = 1 + max_iters * (level - 1); level 2: the initial messages and the messages after every variable update, level 3:
 * after every check update as well; the dump after the last iteration is kept.  The result is
 *     hist[dump][group][x][label]   int64, label < n_labels, x = sent bit of the edge's variable node (0 for the all-zero codeword),
 *                                   group = edge_group[e]; hist_cap = number of int64 the caller's array holds
 * and both calls ADD into hist, so that a caller can loop over batches of any size.  n_labels must be at least the largest
 * message alphabet.  mode decides which (frame, dump) pairs are counted:
 *   0 (all)     every frame at every dump; the exit tests are off for the counted run, as in density evolution
 *   1 (active)  the dumps the reference would have PRINTED for the frame under the decoder's exit conditions, from its lut_decode
 *               return value c: c = 0 none, |c| = max_iters all, 0 < c < max_iters the first (level - 1) * c (it returns before
 *               the dump of its last variable update)
 * The return values come from a normal decode of the batch (any path), which also gives out_bits / out_iters; the messages are
 * then counted in a second pass with the exit tests off (a frame evolves the same whether or not others leave) -- per-class
 * streaming launches, no graph replay.  The exit conditions of the handle are the same before and after the call.
 *
 * set_edge_groups: edge_group[E] in VN-major edge order, values in [0, n_groups); NULL = one group (the default); n_groups 1..256.
 *   ERR_ARG for a count or an id out of range.  Works on a host-only handle (the tables are kept for a later device).
 * histogram_shape: out[4] = {n_dumps for `level`, n_groups, largest message alphabet, E}.
 * histogram_batch: lutldpc_decoder_decode_batch with the counting; sent = host [B*nvar] sent bits or NULL (all-zero codeword);
 *   out_bits / out_iters may be NULL.
 * sim_batch_histogram: sampler (+ encoder) + counted decode for frames frame0 .. frame0+B-1 as lutldpc_decoder_sim_batch sends
 *   them: codewords = host [B*nvar] or NULL; device_codewords != 0: the random codewords of lutldpc_decoder_sim_batch_random.
 * ERR_ARG: level other than 2 / 3, mode other than 0 / 1, n_labels too small, hist_cap short, NULL hist; ERR_STATE: host-only
 * handle, device_codewords without a generator.
 */
int lutldpc_decoder_set_edge_groups(lutldpc_decoder *d, const int32_t *edge_group, int n_groups);
int lutldpc_decoder_histogram_shape(lutldpc_decoder *d, int level, int32_t *out4);
int lutldpc_decoder_histogram_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, const uint8_t *sent, int B, int level, int mode,
                                    int n_labels, uint8_t *out_bits, int32_t *out_iters, int64_t *hist, int64_t hist_cap, int32_t *n_dumps);
int lutldpc_decoder_sim_batch_histogram(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0,
                                        int B, const uint8_t *codewords, int device_codewords, int level, int mode, int n_labels,
                                        int64_t *hist, int64_t hist_cap, int32_t *n_dumps);

/*
 * Failed frames captured on the device (lut_ldpc_amd/csrc/hip/kernels_events.hpp): which variable nodes of a frame were decided
 * wrongly, which checks stayed unsatisfied, how heavy both patterns are and whether the decoder knew -- without the decided bits
 * leaving the device.  Frames are Philox-addressed, so (seed, stream, frame) replays a captured frame exactly.
 *
 * For EVERY frame of the batch the device counts cw_errors (decided bits over all nvar nodes that differ from the sent ones) and
 * unsat_checks (parity checks the decided bits violate).  A frame is SELECTED by `select`:
 *   LUTLDPC_EV_CODEWORD   (0)  cw_errors > 0
 *   LUTLDPC_EV_INFO       (1)  data-bit errors > 0 (what the counters call a frame error)
 *   LUTLDPC_EV_FAILED     (2)  iteration code < 0
 *   LUTLDPC_EV_UNDETECTED (3)  cw_errors > 0 and iteration code >= 0
 * Selected frames get slots in ascending frame order; the first max_frames of them are KEPT and written:
 *   events[slot][8]          {frame offset in the batch, iteration code, cw_errors, data-bit errors, unsat_checks, uncoded errors
 *                             (0 for events_batch: no channel), positions stored, checks stored}; the weights are the true ones
 *                             even where the lists are cut short
 *   positions[slot][max_pos] the wrong nodes, ascending, the first max_pos of them; unused entries -1
 *   checks[slot][max_chk]    the unsatisfied checks, likewise
 * Rows from n_stored on are left untouched.  n_selected = number of selected frames (may exceed max_frames), n_stored = kept.
 * positions / checks may be NULL when their maximum is 0.  node_errors[nvar] / check_fails[nchk] (optional, may be NULL): the
 * number of frames of the batch in which a node is wrong / a check unsatisfied -- over ALL frames, not only the selected ones --
 * ADDED into the caller's arrays, so that a caller can loop over batches.  Everything is integer arithmetic: the result is
 * bit-reproducible, the lists are sorted by construction.
 *
 * events_batch: lutldpc_decoder_decode_batch plus the capture.  sent = host [B*nvar] bits the decided ones are compared with, or
 *   NULL (all-zero codeword); it need not be a codeword.  K_info = number of leading bits counted as data bits.  out_bits /
 *   out_iters may be NULL.
 * sim_batch_events: the frames of lutldpc_decoder_sim_batch (device_codewords = 0; codewords = host [B*nvar] or NULL) or
 *   lutldpc_decoder_sim_batch_random (device_codewords != 0), the same frame_stats, and the capture on top.
 * ERR_ARG: NULL request, NULL events, a negative size, select out of range, NULL positions / checks with a positive maximum, bad
 * B / K_info; ERR_STATE: host-only handle, device_codewords without a generator.
 */
#define LUTLDPC_EV_CODEWORD   0
#define LUTLDPC_EV_INFO       1
#define LUTLDPC_EV_FAILED     2
#define LUTLDPC_EV_UNDETECTED 3
typedef struct {
    int32_t select;
    int32_t max_frames, max_pos, max_chk;
    int32_t *events;        /* [max_frames][8]       */
    int32_t *positions;     /* [max_frames][max_pos] */
    int32_t *checks;        /* [max_frames][max_chk] */
    int64_t *node_errors;   /* [nvar], added into; or NULL */
    int64_t *check_fails;   /* [nchk], added into; or NULL */
    int32_t n_selected;     /* out */
    int32_t n_stored;       /* out */
} lutldpc_event_request;

int lutldpc_decoder_events_batch(lutldpc_decoder *d, const uint8_t *cha, const uint8_t *msg0, const uint8_t *sent, int B, int K_info,
                                 uint8_t *out_bits, int32_t *out_iters, lutldpc_event_request *req);
int lutldpc_decoder_sim_batch_events(lutldpc_decoder *d, const lutldpc_channel_cells *cells, uint64_t seed, uint32_t stream, uint64_t frame0,
                                     int B, const uint8_t *codewords, int device_codewords, int K_info, int32_t *frame_stats,
                                     lutldpc_event_request *req);

/* The decoder's HIP stream (hipStream_t as void*), for callers that enqueue their own work. */
void *lutldpc_decoder_stream(lutldpc_decoder *d);

/* ---- measurement hooks (bench.py) ------------------------------------------------------- */
/* Kernel kinds for the per-kernel timers. */
#define LUTLDPC_K_CN_PASS   0   /* check-node pass (min-sum or CHKTREE)           */
#define LUTLDPC_K_VN_PASS   1   /* variable-node LUT pass                          */
#define LUTLDPC_K_DECISION  2   /* decision-tree pass                              */
#define LUTLDPC_K_SYNDROME  3   /* parity checks                                   */
#define LUTLDPC_K_LAYOUT    4   /* transposes / edge initialisation / state update */
#define LUTLDPC_K_FRONTEND  5   /* channel sampler + error counting                */
#define LUTLDPC_K_FUSED_PASS 6  /* skewed pipeline: check pass of one half + variable pass of the other */
#define LUTLDPC_K_RESIDENT  7   /* LDS-resident decode: all iterations of a batch in one launch */
#define LUTLDPC_K_HISTOGRAM 8   /* message-label histogram of one dump (counted decode)              */
#define LUTLDPC_K_COUNT     9

/* When enabled every launch is bracketed by HIP events recorded on the decoder's stream. */
int lutldpc_decoder_set_profiling(lutldpc_decoder *d, int enable);
/* Accumulated since the last reset: total milliseconds and launch count of one kernel kind.
 * Synchronises the stream. */
int lutldpc_decoder_get_profile(lutldpc_decoder *d, int kind, double *total_ms, int64_t *launches);
int lutldpc_decoder_reset_profile(lutldpc_decoder *d);
/* Bytes of device memory held for a batch of B frames (after the first decode of that size). */
int64_t lutldpc_decoder_device_bytes(lutldpc_decoder *d);
/* Algorithmic description of the kernels actually selected, as a JSON string owned by the
 * handle (kernel names, vector width, message bytes b, tile size). */
const char *lutldpc_decoder_describe(lutldpc_decoder *d);

/* ---- self test of the host-side tree compiler (no GPU needed) ---------------------------- */
/*
 * Evaluates the compiled node program of tree [set][cls] of `kind` (0 VARTREE, 1 CHKTREE,
 * 2 DECTREE) for ONE node on the host, exactly as the device interpreter would, so that the
 * CSE / slot allocation can be checked without a GPU.  in[n_in] are the node's inputs
 * (messages, then the channel label for kind 0/2); out[n_out] the results.  This is a
 * verifier of the compile step only -- no decode path uses it.
 */
int lutldpc_selftest_program_eval(lutldpc_decoder *d, int kind, int set, int cls,
                                  const int32_t *in, int n_in, int32_t *out, int n_out);
/* Number of LUT look-ups of that program per node (after sharing) and for the naive walk. */
int lutldpc_selftest_program_stats(lutldpc_decoder *d, int kind, int set, int cls,
                                   int32_t *n_ops, int32_t *n_ops_naive, int32_t *n_slots);

/* The HIP source jit.hpp generates for a variable (kind 0) / CHKTREE check (kind 1: sign / magnitude look-ups; kind 1 + 32: the
 * full-label program the decoder runs by default) / decision (kind 2) class, as the decoder compiles it -- copied into buf when
 * cap suffices; returns the length needed including the terminator, < 0 on error.  With compile != 0 the
 * source is also compiled for gfx950 with hiprtc (no device needed); a failure returns LUTLDPC_ERR_HIP and
 * leaves the compiler log in lutldpc_last_error(). */
int64_t lutldpc_selftest_jit_source(lutldpc_decoder *d, int kind, int set, int cls, char *buf, int64_t cap, int compile);
/* source of the LDS-resident decode kernel for a batch of G frame groups (info: sets per workgroup, threads, LDS bytes) */
int64_t lutldpc_selftest_resident_source(lutldpc_decoder *d, int G, char *buf, int64_t cap, int compile, int32_t *info);

#ifdef __cplusplus
}
#endif
#endif
