// decoder_packed.hip -- lutldpc_decoder_decode_batch_packed: the host-side batch decode for callers who hold their labels already,
// with the bytes that carry no information taken off the host link -- two labels per byte in, the initial messages derived from
// the channel labels on the device, and a window of the decided bits out at one bit each.  Packed labels -> both row sets ->
// decode_tiles -> packed bits; every decode path decode_tiles picks.  Home of every kernel of kernels_packed.hpp.
#include "decoder_state.hpp"
#include "kernels_packed.hpp"

#pragma GCC visibility push(hidden)

// (see preload_code_objects) this unit's code object
hipError_t preload_packed_kernels() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&packed_bits_out_kernel<2>));
}

// frame-major packed labels of B frames (device, `stride` bytes per frame) -> rows_a = min(label, lim_a) and, with lut_b (device,
// 256 entries), rows_b = lut_b[label]
static int launch_labels_in(lutldpc_decoder *d, const uint8_t *src, size_t stride, bool nibbles, uint8_t *rows_a, uint8_t *rows_b, const uint8_t *lut_b,
                            int B, int G, int lim_a) {
    const dim3 grid((unsigned)((stride + 127) / 128), (unsigned)G);
    const bool vec = stride % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3u) == 0;
#define LABELS_IN(NIB, VEC) PACK_DISPATCH(d, launch_k(packed_labels_in_kernel<PK, NIB, VEC>, grid, dim3(256), 0, d->stream, src, stride, rows_a, rows_b, lut_b, B, d->nvar, lim_a))
    if (nibbles) { if (vec) LABELS_IN(1, 1); else LABELS_IN(1, 0); }
    else { if (vec) LABELS_IN(0, 1); else LABELS_IN(0, 0); }
#undef LABELS_IN
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

// decided bits first .. first + count - 1 of the B frames in d_hard -> dst[B][ceil(count / 32)] (device), one bit each
int launch_bits_out(lutldpc_decoder *d, uint32_t *dst, int B, int G, int first, int count) {
    const int W = (count + 31) / 32;
    PACK_DISPATCH(d, launch_k(packed_bits_out_kernel<PK>, dim3((unsigned)((W + kBitsCols - 1) / kBitsCols), (unsigned)G), dim3(256), 0, d->stream,
                              d->d_hard.p, dst, B, d->nvar, first, count, W));
    LAUNCH_CHECK();
    return LUTLDPC_OK;
}

#pragma GCC visibility pop

extern "C" int lutldpc_decoder_decode_batch_packed(lutldpc_decoder *d, const lutldpc_packed_io *io, const uint8_t *cha, const uint8_t *msg0, int B,
                                                   uint32_t *out_words, int32_t *out_iters) {
    if (!d) return fail(LUTLDPC_ERR_ARG, "NULL decoder");
    if (B <= 0) return fail(LUTLDPC_ERR_ARG, "B must be positive");
    if (!io || !cha) return fail(LUTLDPC_ERR_ARG, "NULL argument");
    if (io->in_format != LUTLDPC_IN_BYTES && io->in_format != LUTLDPC_IN_NIBBLES) return fail(LUTLDPC_ERR_ARG, "in_format must be LUTLDPC_IN_BYTES or LUTLDPC_IN_NIBBLES");
    const bool nibbles = io->in_format == LUTLDPC_IN_NIBBLES;
    const int N = d->nvar, nq_msg = d->Nq_Msg[0];
    const int32_t *map = io->cha2msg_map;
    if ((msg0 != nullptr) == (map != nullptr)) return fail(LUTLDPC_ERR_ARG, "give either msg0 or cha2msg_map");
    if (nibbles && d->Nq_Cha > 16) return fail(LUTLDPC_ERR_ARG, "LUTLDPC_IN_NIBBLES needs a channel alphabet of at most 16 labels");
    if (nibbles && !map && nq_msg > 16) return fail(LUTLDPC_ERR_ARG, "LUTLDPC_IN_NIBBLES with msg0 given needs a first message alphabet of at most 16 labels");
    for (int i = 0; map && i < d->Nq_Cha; i++)
        if (map[i] < 0 || map[i] >= nq_msg) return fail(LUTLDPC_ERR_ARG, "cha2msg_map entry outside [0, Nq_Msg[0])");
    if (io->out_first < 0 || io->out_count < 1 || (int64_t)io->out_first + io->out_count > N) return fail(LUTLDPC_ERR_ARG, "output window outside [0, nvar)");
    int rc = batch_entry(d, B);
    if (rc) return rc;
    // labels in: one staging buffer per array the caller sends
    const size_t stride = nibbles ? ((size_t)N + 1) / 2 : (size_t)N, n = (size_t)B * stride;
    HIP_TRY(d->d_in_cha.alloc(n));
    HIP_TRY(hipMemcpyAsync(d->d_in_cha.p, cha, n, hipMemcpyHostToDevice, d->stream));
    if (msg0) {
        HIP_TRY(d->d_in_msg.alloc(n));
        HIP_TRY(hipMemcpyAsync(d->d_in_msg.p, msg0, n, hipMemcpyHostToDevice, d->stream));
    }
    if ((rc = ensure_batch(d, B))) return rc;
    const int G = d->bpad(B) / d->tile();
    {
        Timed t(d, LUTLDPC_K_LAYOUT);
        if (map) {      // clamp, then map: one table over every value a byte can take
            uint8_t lut[256];
            for (int x = 0; x < 256; x++) lut[x] = (uint8_t)map[std::min(x, d->Nq_Cha - 1)];
            const uint8_t *d_lut = static_cast<const uint8_t *>(dev_param_bytes(d, lut, sizeof(lut)));
            if (!d_lut) return LUTLDPC_ERR_HIP;
            rc = launch_labels_in(d, d->d_in_cha.p, stride, nibbles, d->d_cha_t.p, d->d_msg0_t.p, d_lut, B, G, d->Nq_Cha - 1);
        } else if (!(rc = launch_labels_in(d, d->d_in_cha.p, stride, nibbles, d->d_cha_t.p, nullptr, nullptr, B, G, d->Nq_Cha - 1)))
            rc = launch_labels_in(d, d->d_in_msg.p, stride, nibbles, d->d_msg0_t.p, nullptr, nullptr, B, G, nq_msg - 1);
        if (rc) return rc;
    }
    if ((rc = decode_tiles(d, B))) return rc;
    if (out_words) {
        const int W = (io->out_count + 31) / 32;
        HIP_TRY(d->d_out_words.alloc((size_t)B * (size_t)W));
        {
            Timed t(d, LUTLDPC_K_LAYOUT);
            if ((rc = launch_bits_out(d, d->d_out_words.p, B, G, io->out_first, io->out_count))) return rc;
        }
        if ((rc = copy_to_host(d, out_words, d->d_out_words.p, sizeof(uint32_t) * (size_t)B * (size_t)W))) return rc;
    }
    if (out_iters && (rc = iters_to_host(d, out_iters, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}
