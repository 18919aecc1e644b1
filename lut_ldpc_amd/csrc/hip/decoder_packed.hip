// decoder_packed.hip -- lutldpc_decoder_decode_batch_packed: the host-side batch decode for callers who hold their labels already,
// with the bytes that carry no information taken off the host link -- two labels per byte in, the initial messages derived from
// the channel labels on the device, and a window of the decided bits out at one bit each.  Packed labels -> both row sets ->
// decode_tiles -> packed bits; every decode path decode_tiles picks.  The kernels are those of kernels_layout.hpp (decoder_layout.hip).
#include "decoder_state.hpp"

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
    int rc = check_out_window(d, io->out_first, io->out_count);
    if (rc || (rc = batch_entry(d, B))) return rc;
    // labels in: one staging buffer per array the caller sends
    const size_t stride = nibbles ? ((size_t)N + 1) / 2 : (size_t)N;
    if ((rc = labels_from_host(d, cha, msg0, B, stride)) || (rc = ensure_batch(d, B))) return rc;
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
    if (out_words && (rc = bits_to_caller(d, out_words, false, B, io->out_first, io->out_count))) return rc;
    if (out_iters && (rc = iters_to_host(d, out_iters, B))) return rc;
    HIP_TRY(hipStreamSynchronize(d->stream));
    return LUTLDPC_OK;
}
