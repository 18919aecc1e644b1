// decoder_encode.hip -- the encoder on the device: the handle's generator (dense or sparse triangular), the one host path from
// information bits to code bits (encode_batch), the sent-bit rows of a batch (from the encoder or from the caller's bytes) and
// their C-ABI entries.  Home of every kernel of kernels_encode.hpp and kernels_encode_sparse.hpp.
#include "decoder_state.hpp"
#include "kernels_encode_sparse.hpp"
#include "../host/sparse_generator.hpp"

static_assert(kSparseBlockRows == lut_ldpc::kSparseBlock, "the block of the host's inverse rows is the block of sparse_phase_b_kernel");
using Generator = lutldpc_decoder::Generator;

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_encode_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&encode_random_kernel));
}

// bytes of the bit rows of B frames: every node's row in every frame group of the padded batch
static size_t bit_rows_bytes(const lutldpc_decoder *d, int B) { return (size_t)(d->bpad(B) / d->tile()) * d->nvar * (size_t)(d->tile() / 8); }
static int alloc_sent(lutldpc_decoder *d, int B) { HIP_TRY(d->d_sent.alloc(bit_rows_bytes(d, B))); return LUTLDPC_OK; }
// grid y of the kernels whose waves stride over `items` in steps of `chunk`: four waves per workgroup, 64 workgroups at most
static unsigned wave_chunks_ny(int items, int chunk) { return (unsigned)std::min(64, std::max(1, (items + 4 * chunk - 1) / (4 * chunk))); }

// The sparse form: the parity rows K .. K+R-1 of `rows` (G frame groups, information rows in place) from the information rows --
// phase A (s = A u) and phase B (p = T^-1 s, in place), ordered by the stream
static int launch_sparse_parity(lutldpc_decoder *d, uint8_t *rows, int G) {
    const Generator::Sparse &sp = d->gen.sparse;
    const int K = d->gen.K, R = d->gen.R, N = d->nvar, DW = d->tile() / 32;
    if (R < 1) return LUTLDPC_OK;
    uint32_t *r32 = reinterpret_cast<uint32_t *>(rows);
    const int gpw = 64 / DW;                    // frame groups per wave of phase A
    launch_k(sparse_phase_a_kernel, dim3((unsigned)((R + 3) / 4), (unsigned)((G + gpw - 1) / gpw)), dim3(256), 0, d->stream, sp.a_ptr.p, sp.a_cols.p, K, R, N, G, DW, r32);
    LAUNCH_CHECK();
    launch_k(sparse_phase_b_kernel, dim3((unsigned)(G * (DW / kSparseSliceDwords))), dim3(256), 0, d->stream, sp.order.p, sp.e_ptr.p, sp.e_cols.p, sp.inv.p, K, sp.Rp, N, DW, r32);
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// Where the information bits of a batch come from: the caller's packed words [B][stride] on the device, or (words = null) Philox
// at (seed, stream, frame0 ..).  Where the code bits go: the bit rows `rows` (d_sent), or a window of them as packed words.
struct InfoBits { const uint32_t *words; size_t stride; uint64_t seed; uint32_t stream; uint64_t frame0; };
struct WordWindow { int first, count; uint32_t *out; };

// The one host path from the information bits of B frames to code bits.  Sparse form: the information rows into `rows`, the parity
// rows (where the window reaches them), then the window out.  Dense form: one fused kernel per entry -- encode_random_kernel from
// Philox into `rows`, encode_bits_kernel from the caller's words straight to the window (no rows).
static int encode_batch(lutldpc_decoder *d, const InfoBits &src, int B, uint8_t *rows, const WordWindow *win) {
    const Generator &gen = d->gen;
    const int K = gen.K, R = gen.R, N = d->nvar, Bpad = d->bpad(B), G = Bpad / d->tile();
    const int W128 = (K + 127) / 128, W32 = (K + 31) / 32, Wout = win ? (win->count + 31) / 32 : 0;
    const uint32_t seed_lo = (uint32_t)src.seed, seed_hi = (uint32_t)(src.seed >> 32);
    Timed t(d, LUTLDPC_K_FRONTEND);
    if (gen.form == Generator::SPARSE) {
        const unsigned gx = (unsigned)(Bpad / 64);
        if (src.words)
            launch_k(info_rows_packed_kernel, dim3(gx, wave_chunks_ny(W32, kRowsWordChunk)), dim3(256), 0, d->stream, K, src.words, src.stride, B, N, d->tile(), rows);
        else
            launch_k(info_rows_random_kernel, dim3(gx, wave_chunks_ny(W128, 1)), dim3(256), 0, d->stream, K, seed_lo, seed_hi, src.stream, src.frame0, B, N, d->tile(), rows);
        LAUNCH_CHECK();
        if (!win || win->first + win->count > K)
            if (int rc = launch_sparse_parity(d, rows, G)) return rc;
        if (win) {
            launch_k(rows_window_out_kernel, dim3((unsigned)((B + 63) / 64), wave_chunks_ny(Wout, kRowsWordChunk)), dim3(256), 0, d->stream, rows, B, N, d->tile(), win->first, win->count, win->out);
            LAUNCH_CHECK();
        }
        return LUTLDPC_OK;
    }
    const size_t lds = (size_t)W128 * kEncFrames * 16;
    if (win) {
        // one wave per output word that holds parity rows (at least one information-only word per wave where those are fewer)
        const int c_last = win->first + win->count - 1;
        const int n_par = c_last < K ? 0 : Wout - std::max(0, (K - win->first) / 32);
        const unsigned gx = (unsigned)((B + kEncFrames - 1) / kEncFrames), gy = (unsigned)std::max(1, (std::max(n_par, (Wout - n_par + 7) / 8) + 3) / 4);
        launch_k(encode_bits_kernel, dim3(gx, gy), dim3(256), lds, d->stream, gen.dense.A.p, K, R, gen.dense.W32p, src.words, src.stride, B, win->first, win->count, win->out);
    } else {
        // one wave per parity tile (at least one information word per wave where the tiles are fewer); a workgroup is 64 frames
        const int T = (R + kEncTileRows - 1) / kEncTileRows;
        const unsigned gx = (unsigned)(Bpad / kEncFrames), gy = (unsigned)std::max(1, (std::max(T, (W32 + 7) / 8) + 3) / 4);
        launch_k(encode_random_kernel, dim3(gx, gy), dim3(256), lds, d->stream, gen.dense.A.p, K, R, gen.dense.W32p, seed_lo, seed_hi, src.stream, src.frame0, B, N, d->tile(), rows);
    }
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

int encode_tiles(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B) {
    int rc = require_generator(d, "no generator set: random codewords on the device need lutldpc_decoder_set_generator first");
    if (rc || (rc = alloc_sent(d, B))) return rc;
    return encode_batch(d, InfoBits{nullptr, 0, seed, stream, frame0}, B, d->d_sent.p, nullptr);
}

// d_sent -> frame-major bytes at dst (device, B*N)
static int launch_sent_to_bytes(lutldpc_decoder *d, uint8_t *dst, int B) {
    const size_t n = (size_t)B * d->nvar;
    PACK_DISPATCH(d, launch_k(sent_rows_to_bytes_kernel<PK>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d->stream, d->d_sent.p, B, d->nvar, dst));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

int sent_rows_from_host(lutldpc_decoder *d, const uint8_t *codewords, int B, const uint8_t **rows) {
    *rows = nullptr;
    if (!codewords) return LUTLDPC_OK;
    const int N = d->nvar;
    const size_t n_bytes = bit_rows_bytes(d, B);
    HIP_TRY(d->d_codewords.alloc((size_t)B * N));
    if (int rc = alloc_sent(d, B)) return rc;
    HIP_TRY(hipMemcpyAsync(d->d_codewords.p, codewords, (size_t)B * N, hipMemcpyHostToDevice, d->stream));
    Timed t(d, LUTLDPC_K_LAYOUT);
    PACK_DISPATCH(d, launch_k(bytes_to_sent_rows_kernel<PK>, dim3((unsigned)((n_bytes + 255) / 256)), dim3(256), 0, d->stream, d->d_codewords.p, B, N, n_bytes, d->d_sent.p));
    LAUNCH_CHECK();
    *rows = d->d_sent.p;
    return LUTLDPC_OK;
}

int sent_rows_of(lutldpc_decoder *d, const uint8_t *codewords, bool device_codewords, uint64_t seed, uint32_t stream, uint64_t frame0, int B,
                 const uint8_t **rows) {
    if (!device_codewords) return sent_rows_from_host(d, codewords, B, rows);
    const int rc = encode_tiles(d, seed, stream, frame0, B);
    *rows = d->d_sent.p;
    return rc;
}

// a complete generator replaces the handle's; the move frees the buffers of the one it replaces, whatever its form
static int install_generator(lutldpc_decoder *d, Generator &&gen) {
    HIP_TRY(hipStreamSynchronize(d->stream));           // (a batch in flight may still read the previous generator)
    d->gen = std::move(gen);
    make_describe(d);
    return LUTLDPC_OK;
}

#pragma GCC visibility pop

extern "C" {

int lutldpc_decoder_set_generator(lutldpc_decoder *d, int K, int R, const uint64_t *rows) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (!rows) return fail(LUTLDPC_ERR_ARG, "generator rows are NULL");
    if (K < 1 || R < 0 || K + R != d->nvar) return fail(LUTLDPC_ERR_ARG, "generator: K + R must equal nvar (K >= 1)");
    if (int rc = device_entry(d)) return rc;
    if (K > kEncMaxInfoBits) return fail(LUTLDPC_ERR_UNSUPPORTED, "generator: more than 8192 information bits (limit of the dense device encoder; lutldpc_decoder_set_sparse_generator has none)");
    const int WK = (K + 63) / 64, W32p = 4 * ((K + 127) / 128), Rp = (R + kEncTileRows - 1) / kEncTileRows * kEncTileRows;
    std::vector<uint32_t> a((size_t)std::max(Rp, 1) * W32p, 0u);
    for (int i = 0; i < R; i++)
        for (int j = 0; j < 2 * WK; j++) {
            const int k0 = 32 * j;
            uint32_t w = (uint32_t)(rows[(size_t)i * WK + (size_t)(j >> 1)] >> (32 * (j & 1)));
            if (k0 + 32 > K) w &= k0 >= K ? 0u : (1u << (K - k0)) - 1u;        // bits beyond K stay zero (the info words carry random bits there)
            a[(size_t)i * W32p + (size_t)j] = w;
        }
    Generator gen;                                                     // complete before it replaces the handle's
    gen.form = Generator::DENSE; gen.K = K; gen.R = R; gen.dense.W32p = W32p;
    HIP_TRY(gen.dense.A.upload(a));
    return install_generator(d, std::move(gen));
}

int lutldpc_decoder_set_sparse_generator(lutldpc_decoder *d, int K, int R, const int32_t *row_ptr, const int32_t *cols) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (!row_ptr || !cols) return fail(LUTLDPC_ERR_ARG, "sparse generator: row_ptr or cols is NULL");
    if (K < 1 || R < 0 || K + R != d->nvar) return fail(LUTLDPC_ERR_ARG, "sparse generator: K + R must equal nvar (K >= 1, R >= 0)");
    std::vector<int32_t> order;
    int depth = 0;
    const std::string bad = lut_ldpc::sparse_order(K, R, row_ptr, cols, order, depth);
    if (!bad.empty()) return fail(LUTLDPC_ERR_ARG, "sparse generator: " + bad);
    if (int rc = device_entry(d)) return rc;
    lut_ldpc::SparsePacked P;
    lut_ldpc::sparse_pack(K, R, row_ptr, cols, order, depth, P);
    const std::string oob = lut_ldpc::sparse_packed_check(P);         // every index the kernels follow, before anything reaches the device
    if (!oob.empty()) return fail(LUTLDPC_ERR_STATE, "sparse generator: packed arrays out of bounds (" + oob + ")");
    Generator gen;                                                     // complete before it replaces the handle's
    gen.form = Generator::SPARSE; gen.K = K; gen.R = R;
    Generator::Sparse &up = gen.sparse;
    HIP_TRY(up.a_ptr.upload(P.a_ptr)); HIP_TRY(up.a_cols.upload(P.a_cols)); HIP_TRY(up.order.upload(P.order));
    HIP_TRY(up.e_ptr.upload(P.e_ptr)); HIP_TRY(up.e_cols.upload(P.e_cols)); HIP_TRY(up.inv.upload(P.inv));
    up.Rp = P.Rp; up.depth = P.depth; up.terms = (long long)P.terms(); up.block = kSparseBlockRows;
    return install_generator(d, std::move(gen));
}

int lutldpc_decoder_encode_random(lutldpc_decoder *d, uint64_t seed, uint32_t stream, uint64_t frame0, int B, uint8_t *codewords) {
    int rc = batch_entry(d, B, stream);
    if (rc || (rc = encode_tiles(d, seed, stream, frame0, B))) return rc;
    if (codewords) {
        const size_t n = (size_t)B * d->nvar;
        HIP_TRY(d->d_out_bits.alloc(n));
        if ((rc = launch_sent_to_bytes(d, d->d_out_bits.p, B)) || (rc = copy_to_host(d, codewords, d->d_out_bits.p, n))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

// The caller's information bits -> codewords, bit-packed both ways, in host or device memory.  Works on its own staging buffers
// and the generator alone (the sparse form: on bit rows of its own, d_enc_rows): no label rows, no frame-group state of a decode.
int lutldpc_decoder_encode_packed(lutldpc_decoder *d, const lutldpc_encode_io *io, const uint32_t *info, int B, uint32_t *out_words) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0) return fail(LUTLDPC_ERR_ARG, "B must be positive");
    if (!io || !info || !out_words) return fail(LUTLDPC_ERR_ARG, "NULL argument: io, info and out_words are required");
    if (reinterpret_cast<uintptr_t>(info) % 4 || reinterpret_cast<uintptr_t>(out_words) % 4) return fail(LUTLDPC_ERR_ARG, "info and out_words must be 4-byte aligned");
    const int W32 = (d->gen.K + 31) / 32;             // (a handle without a generator: W32 = 0, and the state error below)
    if (io->in_stride < 0 || (io->in_stride != 0 && io->in_stride < W32)) return fail(LUTLDPC_ERR_ARG, "in_stride must be 0 or at least ceil(K/32)");
    const int Wout = (io->out_count + 31) / 32;
    int rc = check_out_window(d, io->out_first, io->out_count);
    if (rc || (rc = batch_entry(d, B))) return rc;
    if ((rc = require_generator(d, "encode_packed: no generator set (lutldpc_decoder_set_generator)"))) return rc;
    const bool dev = io->on_device != 0;
    InfoBits src{info, io->in_stride ? (size_t)io->in_stride : (size_t)W32, 0, 0, 0};
    WordWindow win{io->out_first, io->out_count, out_words};
    if (d->gen.form == Generator::SPARSE) HIP_TRY(d->d_enc_rows.alloc(bit_rows_bytes(d, B)));
    if (!dev) {         // the whole batch, gaps included, up to the last word read
        const size_t words = (size_t)(B - 1) * src.stride + (size_t)W32;
        HIP_TRY(d->d_host_in.alloc((words + 1) / 2));
        HIP_TRY(hipMemcpyAsync(d->d_host_in.p, info, words * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
        src.words = reinterpret_cast<const uint32_t *>(d->d_host_in.p);
        HIP_TRY(d->d_out_words.alloc((size_t)B * (size_t)Wout));
        win.out = d->d_out_words.p;
    }
    if ((rc = encode_batch(d, src, B, d->d_enc_rows.p, &win))) return rc;
    if (!dev && (rc = copy_to_host(d, out_words, win.out, sizeof(uint32_t) * (size_t)B * (size_t)Wout))) return rc;
    if (!dev || io->sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}

}  // extern "C"
