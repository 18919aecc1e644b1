// ber_sim_multi.cpp -- ber_sim over several MI355X of one node, natively in C++ (BASELINE config 4).
//
// The reference runs one single-threaded process per seed and adds the result files up afterwards
// (scripts/aggregate_results.m:73-84).  Here ONE run of a parameter file shards the frames of every SNR point over the devices:
//   * one host thread, one simulation object (its own codec replica, decoder handle and HIP stream) per *lane*, each running
//     LDPC_BER_Sim::run -- the sweep and the frame loop of the single-device run -- with its rank's view of the exchange below;
//     this file holds what is specific to several ranks: the barrier, RCCL, the exchange, the threads; `lanes` lanes per
//     device (default 2: while lane A's decode occupies the device, lane B's sampler runs and lane A's counters of the batch
//     before go back over PCIe and through the host prefix -- the overlap a double buffer would give, without sharing buffers);
//   * frames are Philox-addressed (kernels_frontend.hpp), so rank r of R simply takes the batch [f0 + r * batch, + batch) of every
//     round; no data-path exchange;
//   * per round two tiny exchanges: all-gather of {frames, frame errors} per rank (2 x int64) and all-reduce of the rank's
//     contribution to the five counters of src/LDPC_BER_Sim.hpp:80-85 -- the batch before the stopping frame whole, the batch
//     containing it truncated, later ones nothing -- so that the stop rule of src/LDPC_BER_Sim.cpp:289 (`> Nfers`) is applied
//     in global frame order and the counters equal those of the frame-by-frame loop (same rule as lut_ldpc_amd/ber_sim.py:73-108 and LDPC_BER_Sim::sim_snr_point);
//   * the exchanges run over RCCL (ncclAllGather / ncclAllReduce on the devices' own communicators, ncclCommInitAll; xGMI between
//     the GPUs of a node) with the lanes of a device folded on the host first; `host` exchange (threads + barrier only) is the
//     rehearsal mode for ranks that share a device, which RCCL refuses.
// librccl is loaded with dlopen: the library itself does not depend on it.
#include "ber_sim_driver.hpp"

#include <hip/hip_runtime_api.h>
#include <dlfcn.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>

namespace lut_ldpc {

namespace {

// ---- a reusable barrier (C++17: no std::barrier)
class Barrier {
public:
    explicit Barrier(int n) : n_(n) {}
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        const int gen = gen_;
        if (++count_ == n_) { count_ = 0; gen_++; cv_.notify_all(); }
        else cv_.wait(lk, [&] { return gen != gen_ || failed_; });
        if (failed_) throw std::runtime_error("another rank failed");
    }
    void fail() { std::lock_guard<std::mutex> lk(mu_); failed_ = true; cv_.notify_all(); }
private:
    std::mutex mu_;
    std::condition_variable cv_;
    int n_, count_ = 0, gen_ = 0;
    bool failed_ = false;
};

// ---- RCCL through dlopen (types as in <rccl/rccl.h>: ncclInt64 = 4, ncclSum = 0)
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*AllReduce)(const void *send, void *recv, size_t count, int dtype, int op, void *comm, hipStream_t s) = nullptr;
    int (*AllGather)(const void *send, void *recv, size_t sendcount, int dtype, void *comm, hipStream_t s) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool load(std::string &err) {
        const char *name = std::getenv("LUTLDPC_RCCL_LIB");
        lib = dlopen(name && *name ? name : "librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib && !(name && *name)) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) { err = std::string("cannot load RCCL: ") + dlerror(); return false; }
        auto sym = [&](const char *s) { void *p = dlsym(lib, s); if (!p) err = std::string("RCCL symbol missing: ") + s; return p; };
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
        AllGather = reinterpret_cast<decltype(AllGather)>(sym("ncclAllGather"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        return CommInitAll && CommDestroy && AllReduce && AllGather && GetErrorString;
    }
};
constexpr int kNcclInt64 = 4, kNcclSum = 0;

// ---- the counter exchange of one run: R = devices x lanes ranks, rank = lane * n_dev + device slot
struct Exchange {
    int n_dev = 1, lanes = 1, R = 1;
    bool use_rccl = false;
    Rccl rccl;
    std::vector<int> devices;
    std::vector<void *> comms;                       // one per device slot
    std::vector<hipStream_t> streams;
    std::vector<int64_t *> d_send, d_recv;           // device buffers of the device leaders
    std::vector<int64_t> gather;                     // [R][2] of the current round
    std::vector<int64_t> reduce_in;                  // [R][5]
    std::vector<int64_t> reduce_out;                 // [5]
    std::unique_ptr<Barrier> bar;
    std::vector<std::unique_ptr<Barrier>> dev_bar;   // the lanes of one device

    void hip_check(hipError_t e, const char *what) { if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); }
    void nccl_check(int rc, const char *what) { if (rc != 0) throw std::runtime_error(std::string(what) + ": " + rccl.GetErrorString(rc)); }

    void init(const std::vector<int> &devs, int lanes_, const std::string &mode) {
        devices = devs; n_dev = (int)devs.size(); lanes = lanes_; R = n_dev * lanes;
        gather.assign((size_t)R * 2, 0); reduce_in.assign((size_t)R * 5, 0); reduce_out.assign(5, 0);
        bar.reset(new Barrier(R));
        for (int i = 0; i < n_dev; i++) dev_bar.emplace_back(new Barrier(lanes));
        bool distinct = true;
        for (int i = 0; i < n_dev; i++) for (int j = 0; j < i; j++) distinct = distinct && devs[(size_t)i] != devs[(size_t)j];
        if (mode == "host" || (mode == "auto" && (!distinct || n_dev == 1))) return;
        if (!distinct) throw std::runtime_error("RCCL needs one device per rank: the device list repeats a device (use --exchange host to rehearse)");
        std::string err;
        if (!rccl.load(err)) { if (mode == "rccl") throw std::runtime_error(err); std::cerr << "ber_sim: " << err << " -- counters are exchanged on the host\n"; return; }
        comms.assign((size_t)n_dev, nullptr);
        nccl_check(rccl.CommInitAll(comms.data(), n_dev, devices.data()), "ncclCommInitAll");
        streams.assign((size_t)n_dev, nullptr); d_send.assign((size_t)n_dev, nullptr); d_recv.assign((size_t)n_dev, nullptr);
        for (int i = 0; i < n_dev; i++) {
            hip_check(hipSetDevice(devices[(size_t)i]), "hipSetDevice");
            hip_check(hipStreamCreateWithFlags(&streams[(size_t)i], hipStreamNonBlocking), "hipStreamCreate");
            hip_check(hipMalloc((void **)&d_send[(size_t)i], sizeof(int64_t) * (size_t)(5 + 2 * lanes)), "hipMalloc");
            hip_check(hipMalloc((void **)&d_recv[(size_t)i], sizeof(int64_t) * (size_t)(5 + 2 * R)), "hipMalloc");
        }
        use_rccl = true;
    }
    void destroy() {
        for (size_t i = 0; i < comms.size(); i++) {
            (void)hipSetDevice(devices[i]);
            if (d_send[i]) (void)hipFree(d_send[i]);
            if (d_recv[i]) (void)hipFree(d_recv[i]);
            if (streams[i]) (void)hipStreamDestroy(streams[i]);
            if (comms[i]) (void)rccl.CommDestroy(comms[i]);
        }
        comms.clear();
    }

    // every rank contributes mine[2]; afterwards all[R][2] holds every rank's pair, in rank order
    void all_gather2(int rank, const int64_t *mine, int64_t *all) {
        const int slot = rank % n_dev, lane = rank / n_dev;
        gather[(size_t)rank * 2] = mine[0]; gather[(size_t)rank * 2 + 1] = mine[1];
        if (use_rccl) {
            dev_bar[(size_t)slot]->wait();                                 // the lanes of this device have written their pairs
            if (lane == 0) {
                // payload of this device: its lanes' pairs; gathered order = [device slot][lane]
                std::vector<int64_t> h((size_t)2 * lanes), g((size_t)2 * R);
                for (int l = 0; l < lanes; l++) { h[(size_t)2 * l] = gather[(size_t)(l * n_dev + slot) * 2]; h[(size_t)2 * l + 1] = gather[(size_t)(l * n_dev + slot) * 2 + 1]; }
                hip_check(hipSetDevice(devices[(size_t)slot]), "hipSetDevice");
                hip_check(hipMemcpyAsync(d_send[(size_t)slot], h.data(), sizeof(int64_t) * h.size(), hipMemcpyHostToDevice, streams[(size_t)slot]), "hipMemcpyAsync");
                nccl_check(rccl.AllGather(d_send[(size_t)slot], d_recv[(size_t)slot], (size_t)2 * lanes, kNcclInt64, comms[(size_t)slot], streams[(size_t)slot]), "ncclAllGather");
                hip_check(hipMemcpyAsync(g.data(), d_recv[(size_t)slot], sizeof(int64_t) * g.size(), hipMemcpyDeviceToHost, streams[(size_t)slot]), "hipMemcpyAsync");
                hip_check(hipStreamSynchronize(streams[(size_t)slot]), "hipStreamSynchronize");
                if (slot == 0)       // one writer puts what came over the links into the shared table (every device received the same)
                    for (int s2 = 0; s2 < n_dev; s2++) for (int l = 0; l < lanes; l++) { gather[(size_t)(l * n_dev + s2) * 2] = g[(size_t)(s2 * lanes + l) * 2]; gather[(size_t)(l * n_dev + s2) * 2 + 1] = g[(size_t)(s2 * lanes + l) * 2 + 1]; }
            }
        }
        bar->wait();
        std::memcpy(all, gather.data(), sizeof(int64_t) * (size_t)R * 2);
        bar->wait();                                                       // nobody overwrites the table before everybody has read it
    }
    // sum of every rank's v[5], returned in v on every rank
    void all_reduce5(int rank, int64_t *v) {
        const int slot = rank % n_dev, lane = rank / n_dev;
        std::memcpy(&reduce_in[(size_t)rank * 5], v, sizeof(int64_t) * 5);
        if (use_rccl) {
            dev_bar[(size_t)slot]->wait();
            if (lane == 0) {
                int64_t h[5] = {0, 0, 0, 0, 0}, g[5];
                for (int l = 0; l < lanes; l++) for (int k = 0; k < 5; k++) h[k] += reduce_in[(size_t)(l * n_dev + slot) * 5 + (size_t)k];
                hip_check(hipSetDevice(devices[(size_t)slot]), "hipSetDevice");
                hip_check(hipMemcpyAsync(d_send[(size_t)slot], h, sizeof(h), hipMemcpyHostToDevice, streams[(size_t)slot]), "hipMemcpyAsync");
                nccl_check(rccl.AllReduce(d_send[(size_t)slot], d_recv[(size_t)slot], 5, kNcclInt64, kNcclSum, comms[(size_t)slot], streams[(size_t)slot]), "ncclAllReduce");
                hip_check(hipMemcpyAsync(g, d_recv[(size_t)slot], sizeof(g), hipMemcpyDeviceToHost, streams[(size_t)slot]), "hipMemcpyAsync");
                hip_check(hipStreamSynchronize(streams[(size_t)slot]), "hipStreamSynchronize");
                if (slot == 0) std::memcpy(reduce_out.data(), g, sizeof(g));
            }
            bar->wait();
        } else {
            bar->wait();
            if (rank == 0) for (int k = 0; k < 5; k++) { int64_t s = 0; for (int r = 0; r < R; r++) s += reduce_in[(size_t)r * 5 + (size_t)k]; reduce_out[(size_t)k] = s; }
            bar->wait();
        }
        std::memcpy(v, reduce_out.data(), sizeof(int64_t) * 5);
        bar->wait();
    }
};

// rank `rank` of the run's exchange, as the frame loop sees it
struct RankExchange : CounterExchange {
    RankExchange(Exchange &ex_, int rank_) : CounterExchange(rank_, ex_.R), ex(ex_) {}
    void all_gather2(const int64_t *mine, int64_t *all) const override { ex.all_gather2(rank, mine, all); }
    void all_reduce5(int64_t *v) const override { ex.all_reduce5(rank, v); }
    std::string layout() const override {
        return " on " + std::to_string(ex.n_dev) + " device(s) x " + std::to_string(ex.lanes) + " lane(s), counters over " + (ex.use_rccl ? "RCCL" : "the host");
    }
    Exchange &ex;
};

}  // namespace

int ber_sim_run_multi(const std::string &params_path, const std::string &base_dir, int seed, const std::string &custom_name,
                      const std::vector<int> &devices, int lanes, const std::string &exchange_mode, bool quiet) {
    if (devices.empty() || lanes < 1 || lanes > 8) throw std::runtime_error("ber_sim: need at least one device and 1..8 lanes");
    Exchange ex;
    ex.init(devices, lanes, exchange_mode);
    const int R = ex.R;
    std::vector<std::unique_ptr<LDPC_BER_Sim>> sims((size_t)R);
    std::vector<std::string> errors((size_t)R);
    std::atomic<bool> failed{false};
    Barrier start(R);
    auto worker = [&](int rank) {
        try {
            sims[(size_t)rank] = make_ber_sim(params_path, base_dir, seed, custom_name, devices[(size_t)(rank % ex.n_dev)]);
            LDPC_BER_Sim &S = *sims[(size_t)rank];
            S.quiet = quiet;
            S.codec_writer = rank == 0;                              // one rank writes lut_codec.it
            S.load();
            start.wait();
            S.run(RankExchange(ex, rank));                           // src/LDPC_BER_Sim.cpp:121-155 on every rank, same decisions everywhere
        } catch (const std::exception &e) {
            errors[(size_t)rank] = e.what();
            failed = true;
            start.fail(); ex.bar->fail();
            for (auto &b : ex.dev_bar) b->fail();
        }
    };
    std::vector<std::thread> pool;
    for (int r = 1; r < R; r++) pool.emplace_back(worker, r);
    worker(0);
    for (auto &t : pool) t.join();
    ex.destroy();
    if (failed) {
        std::string msg;
        for (int r = 0; r < R; r++) if (!errors[(size_t)r].empty() && errors[(size_t)r] != "another rank failed") msg += "rank " + std::to_string(r) + ": " + errors[(size_t)r] + "; ";
        throw std::runtime_error(msg.empty() ? "a rank failed" : msg);
    }
    sims[0]->save();
    return 0;
}

}  // namespace lut_ldpc
