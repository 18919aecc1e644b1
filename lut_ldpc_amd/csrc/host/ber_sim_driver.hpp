// ber_sim_driver.hpp -- LDPC_BER_Sim / LDPC_BER_Sim_LUT / LDPC_BER_Sim_Results: the Monte-Carlo
// driver of the reference (src/LDPC_BER_Sim.hpp:57-215) with the frame loop batched on the GPU.
//
// Same parameter file, same public fields and methods (load / run / save / sim_snr_point /
// gen_filename / append_custom_name), same results file.  What changes underneath:
//   * frames are simulated in batches through lutldpc_decoder_sim_batch (sampler + decode + error
//     counting on the device); the stop rule of sim_snr_point (src/LDPC_BER_Sim.cpp:289: stop once
//     MORE than Nfers frame errors were seen) is applied to the per-frame results in frame order,
//     so the counters are exactly what a frame-by-frame loop over the same frames would give;
//   * random numbers are Philox-addressed per (seed, SNR index, frame), see kernels_frontend.hpp;
//   * the [BP] branch (IT++'s own BP decoder, src/LDPC_BER_Sim.cpp:157-244) is LDPC_BER_Sim_BP: the comparison decoder of
//     include/lut_ldpc_bp.h on the device behind a host AWGN front end, or (BP.front_end = device) with its channel and error
//     counters on the device as well (PARITY UNPINNED: the IT++ fork is absent).
#pragma once
#include "ldpc_code_lut.hpp"
#include "lut_ldpc_hip.h"
#include "lut_ldpc_bp.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <optional>
#include <string>
#include <vector>

namespace lut_ldpc {

// src/LDPC_BER_Sim.hpp:57-88
class LDPC_BER_Sim_Results {
public:
    LDPC_BER_Sim_Results() = default;
    LDPC_BER_Sim_Results(int nvar, int nchk) : ldpc_nvar(nvar), ldpc_nchk(nchk), ldpc_code_rate(1.0 - (double)nchk / nvar) {}
    void add_snr_point(double snr, int64_t frames, int64_t databits, int64_t frame_errors, int64_t data_bit_errors, int64_t uncoded_bit_errors);
    void save_runtime(double t) { runtime = t; }
    void write_itfile(const std::string &filename) const;       // src/LDPC_BER_Sim.cpp:342-362
    std::vector<double> sim_SNRdB;
    std::vector<int64_t> sim_Nframes, sim_Ndatabits, sim_frame_errors, sim_data_bit_errors, sim_uncoded_bit_errors;
    int ldpc_nvar = 0, ldpc_nchk = 0;
    double ldpc_code_rate = 0, runtime = 0;
    // written only where the parameter file gave the two Channel keys: the class of every node, the SNR offset of every class
    std::vector<double> channel_node_classes, channel_class_snr_offset_dB;
};

// The received-value partition handed to the device sampler (see kernels_frontend.hpp).
struct ChannelCellTable {
    std::vector<uint64_t> thr;
    std::vector<uint8_t> cha, msg, neg, cha_m, msg_m;
    lutldpc_channel_cells view() const;
};
// N0: noise spectral density (variance N0/2 per dimension), boundaries in the LLR domain; mode as
// LDPC_Code_LUT::initial_message_mode_t (QCHA derives the message label from the channel label)
ChannelCellTable make_channel_cells(double N0, const vec &qb_Cha, const vec &qb_Msg, int initial_message_mode, const ivec &cha2msg_map);

// floor(2^64 * P(x <= t)) for x ~ N(1, sigma^2), the nearer tail through erfc, raised to `previous` (the running maximum of a
// table): the one routine behind every cumulative cell probability, of the LUT table above and of the [BP] table below
uint64_t cumulative_threshold(double t, double sigma, uint64_t previous);

// The [BP] front end's cells (include/lut_ldpc_bp.h: lutldpc_bp_cells, lutldpc_bp_awgn_cells): a cell per QLLR value of
// to_qllr(4x/N0) with x ~ N(1, N0/2), QLLR 0 split at x = 0, zero-mass ends trimmed
struct BpCellTable {
    std::vector<uint64_t> thr;
    std::vector<int32_t> qllr;
    std::vector<uint8_t> neg;
    lutldpc_bp_cells view() const { return lutldpc_bp_cells{(int32_t)qllr.size(), thr.data(), qllr.data(), neg.data()}; }
};
// the number of cells of that table without building it; the kept thresholds are k_first .. k_last (cells k_first .. k_last + 1)
int64_t bp_awgn_cell_count(int d1, int d4, double N0, int64_t *k_first, int64_t *k_last, bool *zero_split);
// throws std::length_error above LUTLDPC_BP_MAX_CELLS
BpCellTable make_bp_awgn_cells(int d1, int d4, double N0);

// N0 of an SNR point: Eb/N0 = SNRdB at unit bit energy (src/LDPC_BER_Sim.cpp:248)
inline double noise_n0(double snr_db, double code_rate) { return std::pow(10.0, -snr_db / 10.0) / code_rate; }
// the cell table of codec C at this SNR
ChannelCellTable channel_cells_at(const LDPC_Code_LUT &C, double snr_db);

// Per-node channel classes as the codec layer holds them (include/lut_ldpc_host.h: lutldpc_codec_set_node_channels; ber_sim:
// Channel.node_classes_filename / Channel.class_snr_offset_dB): the class of every node and, per class, an SNR offset in dB.  The
// table of class c at an SNR point is that of the code at snr_db + offset_db[c]; -inf is a punctured node (an erasure), +inf a
// known bit.  Nothing else is rescaled: N0 stays noise_n0(snr, code rate), a user who punctures accounts for the effective rate.
struct NodeChannelClasses {
    std::vector<uint8_t> node_class;     // nvar ids, in the decoder's column order
    std::vector<double> offset_db;       // empty = no classes
    bool set() const { return !offset_db.empty(); }
};
// throws std::invalid_argument: n_classes outside 1 .. LUTLDPC_MAX_NODE_CLASSES, a NaN offset, an id >= n_classes; `what` opens the message
void check_node_channel_classes(const uint8_t *node_class, int nvar, int n_classes, const double *offset_db, const std::string &what);
// channel_cells_at(C, snr_db + offset_db) and its two limits, the limits of make_channel_cells:
//   -inf  two cells, thr = {2^63}: x = 0- (cha = #{qb_Cha < 0}, neg = 1) and x = 0+ (cha = #{qb_Cha <= 0}, neg = 0)
//   +inf  one cell: the top labels, neg = 0
// msg counts qb_Msg the same way (CONT) or is map[cha] (QCHA); mirrors as make_channel_cells makes them
ChannelCellTable node_channel_cells_at(const LDPC_Code_LUT &C, double snr_db, double offset_db);
// The cells the four codec entries that sample hand to the decoder for one SNR point: without classes the code's one table;
// with classes the per-class tables are set on the handle (lutldpc_decoder_set_node_channels) and cells() is NULL.
struct PointCells {
    const lutldpc_channel_cells *cells() const { return classes ? nullptr : &view; }
    ChannelCellTable one;
    lutldpc_channel_cells view{};
    bool classes = false;
};
// returns the code of the setter (LUTLDPC_OK without classes); `pc` must stay where it is while its cells() are in use
int set_point_cells(LDPC_Code_LUT &C, const NodeChannelClasses &nc, double snr_db, PointCells &pc);

// Philox4x32-10 block of (counter, seed): the host twin of the device generator (kernels_frontend.hpp)
void philox4x32_10(uint32_t (&counter)[4], uint64_t seed);
// Philox-addressed data bits of frame f (zero_codeword = false), shared with the tests
void random_info_bits(uint64_t seed, uint32_t stream, uint64_t frame, int K, unsigned char *out);
// the codewords of frames frame0 .. frame0+B-1 made on the host (random_info_bits + enc.encode): B rows of N bytes
template <class Encoder>
std::vector<unsigned char> random_codewords(Encoder &enc, uint64_t seed, uint32_t stream, uint64_t frame0, int B, int N, int K) {
    std::vector<unsigned char> codewords((size_t)B * N);
    bvec info((size_t)K), cw;
    for (int i = 0; i < B; i++) {
        random_info_bits(seed, stream, frame0 + (uint64_t)i, K, info.data());
        enc.encode(info, cw);
        std::copy_n(cw.data(), (size_t)N, &codewords[(size_t)i * N]);
    }
    return codewords;
}

// per-frame result of one simulated frame: {lut_decode code, frame error, data bit errors, uncoded errors}
struct FrameStats { int32_t iters, frame_error, bit_errors, uncoded_errors; };

// The counter exchange of the frame loop: rank `rank` of `ranks` takes every ranks-th batch of an SNR point and meets the others
// twice per round.  This class is the single-rank exchange (no threads, no barrier, no HIP call); ber_sim_multi.cpp overrides it
// for the lanes and devices of one run -- a rank that cannot complete an exchange there throws, which is how "another rank
// failed" reaches the frame loop.
class CounterExchange {
public:
    explicit CounterExchange(int rank_ = 0, int ranks_ = 1) : rank(rank_), ranks(ranks_) {}
    virtual ~CounterExchange() = default;
    // every rank contributes mine[2]; afterwards all[ranks][2] holds every rank's pair, in rank order
    virtual void all_gather2(const int64_t *mine, int64_t *all) const { all[0] = mine[0]; all[1] = mine[1]; }
    // sum of every rank's v[5], returned in v on every rank
    virtual void all_reduce5(int64_t *) const {}
    // what the closing line of run() says between "Done simulating" and ". Runtime"
    virtual std::string layout() const { return ""; }
    const int rank, ranks;
};

class LDPC_BER_Sim {
public:
    LDPC_BER_Sim(const std::string &params_file_path, const std::string &base_dir_path);   // src/LDPC_BER_Sim.cpp:42-102
    virtual ~LDPC_BER_Sim() = default;
    virtual void load() = 0;
    // every rank of `ex` runs the same sweep and takes the same decisions; rank 0 prints
    virtual void run(const CounterExchange &ex = CounterExchange());   // :121-155
    virtual void save();                                         // :317-340
    std::string results_file_path() const;                       // <results_dir>/<gen_filename>/<gen_filename>_rseedNNNN.it
    virtual bool sim_snr_point(double snr, int snr_index) { return sim_snr_point(snr, snr_index, CounterExchange()); }   // :246-311
    // the frame loop, batched through sim_batch and sharded over the ranks of `ex`: rank r takes the batch [f0 + r * batch, + batch)
    // of every round, and the stop rule of :289 is applied in global frame order, so the counters are those of the frame-by-frame loop
    bool sim_snr_point(double snr, int snr_index, const CounterExchange &ex);
    // frames frame0 .. frame0+B-1 of SNR point `snr_index` (any order, any sharding): the body of the
    // frame loop, :262-286.  The stop rule is applied by the caller (sim_snr_point).
    virtual void sim_batch(double snr, int snr_index, int64_t frame0, int B, FrameStats *stats) = 0;
    // message-label histograms of the same frames (lutldpc_decoder_sim_batch_histogram), added into hist; returns its code
    virtual int message_histogram(double, int, int64_t, int, int, int, int, int64_t *, int64_t, int32_t *) {
        throw std::logic_error("message histograms exist for [LUT] simulations only");
    }
    // failed frames of the same frames, captured on the device (lutldpc_decoder_sim_batch_events); returns its code
    virtual int error_events(double, int, int64_t, int, lutldpc_event_request *) { throw std::logic_error("error events exist for [LUT] simulations only"); }
    int get_codeword_length() const { return codeword_length; }
    int get_dataword_length() const { return dataword_length; }
    virtual std::string gen_filename() const;                    // :104-115
    void append_custom_name(const std::string &ext) { custom_name += ext; }

    // public parameter fields, as in the reference
    int rand_seed = 0;
    vec SNRdB;
    double Nframes = 1e5;
    int Nfers = 20;
    double ber_min = 1e-7, fer_min = 1e-5;
    int rand_seed_offset = 0, save_codec = 0;
    std::string custom_name, results_prefix = "RES", results_dir = "results", codes_dir = "codes", codec_filename, parity_filename;
    bool zero_codeword = true, save_permuted = false, parity_check_iter = true;
    std::string generator_form = "auto";     // LDPC.generator_form: auto (dense where the matrix is small enough, else sparse) or sparse
    // Channel.node_classes_filename (a text file of nvar class ids under codes_dir) and Channel.class_snr_offset_dB (one offset per
    // class; inf = known bit, -inf = punctured): both or neither.  [LUT] only; the ids are read by load(), which knows nvar
    std::string node_classes_filename;
    vec class_snr_offset_dB;
    int max_iter = 30;
    LDPC_BER_Sim_Results results;
    // build-side knobs
    int device = 0;
    int batch_frames = 32768;        // frames per device call (upper bound; INI key Sim.batch_frames)
    bool quiet = false;
    bool codec_writer = true;        // load() writes lut_codec.it when rand_seed == save_codec (:512); false on all ranks of a run but one

protected:
    // H from <codes_dir>/<parity_filename>.alist and, for zero_codeword = false, G from <parity_filename>.gen.it or constructed
    // from H (save_permuted: both written back), :436-470 and :159-190
    void load_parity_and_generator();
    std::string params_file_path, base_dir, codes_path, results_path;
    int codeword_length = 0, dataword_length = 0;
    bool decoder_set = false, encoder_set = false;
    double code_rate = 0;
    std::unique_ptr<LDPC_Parity> H;
    std::unique_ptr<LDPC_Generator_Systematic> G;
};

class LDPC_BER_Sim_LUT : public LDPC_BER_Sim {
public:
    LDPC_BER_Sim_LUT(const std::string &params_file_path, const std::string &base_dir_path);   // src/LDPC_BER_Sim.cpp:376-430
    void load() override;                                        // :434-550
    void sim_batch(double snr, int snr_index, int64_t frame0, int B, FrameStats *stats) override;
    int message_histogram(double snr, int snr_index, int64_t frame0, int B, int level, int mode, int n_labels, int64_t *hist, int64_t hist_cap,
                          int32_t *n_dumps) override;
    int error_events(double snr, int snr_index, int64_t frame0, int B, lutldpc_event_request *req) override;
    std::string gen_filename() const override;                   // :553-568
    LDPC_Code_LUT *codec() { return C.get(); }

    std::optional<double> design_thr, design_SNRdB;
    int decoder_output_verbosity = 0;
    std::string initial_message_mode = "from_continuous_input", tree_mode = "auto_bin_balanced", trees_dir = "trees", trees_filename;
    int Nq_Cha = 16;
    ivec Nq_Msg;
    bool min_lut = true;
    bvec reuse_lut;
    bool allow_degree_one = false;   // LUT.allow_degree_one (build-side extension, default off = reference behaviour)
    int known_rank = 0;              // LDPC.known_rank (build-side: skip the GF(2) rank computation)

private:
    void load_node_classes();        // Channel.node_classes_filename -> node_channels, checked against nvar and the offsets
    // set_point_cells once per SNR point: the class tables depend on the point alone, so a batch of the point that the handle
    // already holds the tables of sets nothing (as LDPC_BER_Sim_BP keeps one cell table per point)
    int point_cells(double snr, int snr_index, PointCells &pc);
    const lutldpc_decoder *classes_on = nullptr;     // the handle and the point whose class tables it holds
    int classes_snr_index = -1;
    std::string trees_path;
    std::unique_ptr<LDPC_Code_LUT> C;
    NodeChannelClasses node_channels;
};

// BPSK over AWGN in double precision on the host, Philox-addressed per (seed, stream = SNR index, frame, bit pair), Box-Muller:
// llr[i*N + v] = 4 x / N0 with x = (1 - 2 bit) + sqrt(N0/2) z  (src/LDPC_BER_Sim.cpp:270-279, BPSK::demodulate_soft_bits);
// codewords: B*N sent bits or NULL for the all-zero codeword; uncoded[i] = slicer errors of frame i (:283).
void awgn_llr_frames(uint64_t seed, uint32_t stream, uint64_t frame0, int B, int N, double N0, const unsigned char *codewords,
                     double *llr, int32_t *uncoded);

// The reference's base class as it is used for the [BP] section (src/LDPC_BER_Sim.cpp:157-244): itpp::LDPC_Code with
// LLR_calc_unit(qllr_scale_res, qllr_table_size, qllr_spacing_res, qllr_total_res) -> lutldpc_bp_decoder.
class LDPC_BER_Sim_BP : public LDPC_BER_Sim {
public:
    LDPC_BER_Sim_BP(const std::string &params_file_path, const std::string &base_dir_path);   // :42-102
    ~LDPC_BER_Sim_BP() override;
    void load() override;                                        // :157-244
    void sim_batch(double snr, int snr_index, int64_t frame0, int B, FrameStats *stats) override;
    int llr_calc_d1 = 12, llr_calc_d2 = 300, llr_calc_d3 = 7, llr_calc_d4 = 28;                // :75-78
    std::string front_end = "host";  // BP.front_end (build-side): host = awgn_llr_frames + host counters, device = lutldpc_bp_sim_batch
    lutldpc_bp_decoder *decoder() { return dec; }

private:
    lutldpc_bp_decoder *dec = nullptr;
    int cells_snr_index = -1;        // the SNR point whose cell table the decoder holds (device front end)
};

// One run of a parameter file over several devices of a node (ber_sim_multi.cpp): `lanes` host threads per device, each with its
// own simulation object / decoder handle / stream; frames sharded by rank, counters exchanged over RCCL ("rccl"), on the host
// ("host": ranks may share a device) or whichever applies ("auto").  Writes the same result file as the single-device run.
int ber_sim_run_multi(const std::string &params_path, const std::string &base_dir, int seed, const std::string &custom_name,
                      const std::vector<int> &devices, int lanes, const std::string &exchange_mode, bool quiet);

// prog/ber_sim.cpp:128-142: the section present in the parameter file (or Sim.codec_type) picks the simulation class; the object
// comes back with its seed, custom name and device set, ready for load()
std::unique_ptr<LDPC_BER_Sim> make_ber_sim(const std::string &params_path, const std::string &base_dir, int seed = 0,
                                           const std::string &custom_name = "", int device = 0);

// ber_sim's main (prog/ber_sim.cpp:46-160): returns the process exit code
int ber_sim_main(int argc, char **argv);

}  // namespace lut_ldpc
