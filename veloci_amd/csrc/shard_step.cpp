// The sharded step behind include/veloci_amd.h: the RCCL loader and the communicator (vq_comm_*), vq_shard_step_begin / _end / _flat.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include <dlfcn.h>
#include <unistd.h>

#include "capi_internal.hpp"

using namespace vq;
using vqreq::Request;

extern "C" {

// ------------------------------------------------------------------ the sharded step inside the library
// compile -> scans (scan stream) -> all-gather of the packed partials + all-reduce of the facet histograms (RCCL, collective stream) ->
// merge + download (finish stream): one call per step, no interpreter and no tensor library between the stages.  RCCL is loaded at run time
// (librccl.so.1 — the copy already in the process when the caller's framework brought one).
namespace {
typedef struct ncclComm* ncclComm_t;
struct NcclId {
    char internal[VQ_COMM_ID_BYTES];
};
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, NcclId, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*CommAbort)(ncclComm_t) = nullptr;                 // optional
    int (*CommGetAsyncError)(ncclComm_t, int*) = nullptr;   // optional
    const char* (*GetErrorString)(int) = nullptr;
};
constexpr int kNcclUint8 = 1, kNcclUint32 = 3, kNcclUint64 = 5, kNcclSum = 0;  // ncclDataType_t / ncclRedOp_t (rccl.h)
static Rccl& rccl_api() {
    static Rccl r = [] {
        Rccl x;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            x.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (x.h) break;
        }
        if (!x.h) return x;
        auto sym = [&](const char* n) { return dlsym(x.h, n); };
        x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(sym("ncclGetUniqueId"));
        x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(sym("ncclCommInitRank"));
        x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(sym("ncclCommDestroy"));
        x.AllGather = reinterpret_cast<decltype(x.AllGather)>(sym("ncclAllGather"));
        x.AllReduce = reinterpret_cast<decltype(x.AllReduce)>(sym("ncclAllReduce"));
        x.CommAbort = reinterpret_cast<decltype(x.CommAbort)>(sym("ncclCommAbort"));
        x.CommGetAsyncError = reinterpret_cast<decltype(x.CommGetAsyncError)>(sym("ncclCommGetAsyncError"));
        x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(sym("ncclGetErrorString"));
        return x;
    }();
    if (!r.h || !r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.AllReduce)
        throw VelociError(VQ_ERR_DEVICE, "RCCL (librccl.so.1) is not available: the in-library exchange of a sharded step needs it");
    return r;
}
// RCCL greets on stdout when it starts up: a host program's stdout is not this library's to write to (the greeting goes to stderr)
int quiet_stdout(const std::function<int()>& f) {
    std::fflush(stdout);
    const int keep = dup(1);
    if (keep >= 0) (void)dup2(2, 1);
    const int rc = f();
    std::fflush(stdout);
    if (keep >= 0) {
        (void)dup2(keep, 1);
        (void)close(keep);
    }
    return rc;
}
void nccl_check(int rc, const char* what) {
    if (rc != 0) throw VelociError(VQ_ERR_DEVICE, std::string(what) + ": " + (rccl_api().GetErrorString ? rccl_api().GetErrorString(rc) : "RCCL error"));
}
// sums over the shards before compilation (result sizes of count pre-passes, merged list lengths): the in-library form of vq_index_set_allreduce
int comm_sum_u64(void* ctx, uint64_t* values, size_t n) {
    const Index& idx = *static_cast<const Index*>(ctx);
    ShardComm& c = *idx.comm;
    std::lock_guard<std::mutex> g(c.mu);
    try {
        VQ_HIP(hipSetDevice(idx.device));
        c.red.ensure(n * 8);
        VQ_HIP(hipMemcpyAsync(c.red.p, values, n * 8, hipMemcpyHostToDevice, c.stream));
        nccl_check(rccl_api().AllReduce(c.red.p, c.red.p, n, kNcclUint64, kNcclSum, static_cast<ncclComm_t>(c.nccl), c.stream), "ncclAllReduce");
        VQ_HIP(hipMemcpyAsync(values, c.red.p, n * 8, hipMemcpyDeviceToHost, c.stream));
        VQ_HIP(hipStreamSynchronize(c.stream));
        return 0;
    } catch (...) {
        return -1;
    }
}
void comm_setup(Index& idx, std::unique_ptr<ShardComm> c) {
    VQ_HIP(hipSetDevice(idx.device));
    {
        int lo = 0, hi = 0;
        VQ_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        VQ_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));  // (collectives are short and latency-bound: ahead of the next step's scans)
    }
    for (int k = 0; k < 2; ++k) {
        VQ_HIP(hipEventCreateWithFlags(&c->ev_scan[k], hipEventDisableTiming));
        VQ_HIP(hipEventCreateWithFlags(&c->ev_xchg[k], hipEventDisableTiming));
        VQ_HIP(hipEventCreateWithFlags(&c->ev_fin[k], hipEventDisableTiming));
    }
    idx.comm = std::move(c);
}
}  // namespace

vq::ShardComm::~ShardComm() {
    if (nccl) (void)rccl_api().CommDestroy(static_cast<ncclComm_t>(nccl));
    for (int k = 0; k < 2; ++k) {
        if (ev_scan[k]) (void)hipEventDestroy(ev_scan[k]);
        if (ev_xchg[k]) (void)hipEventDestroy(ev_xchg[k]);
        if (ev_fin[k]) (void)hipEventDestroy(ev_fin[k]);
    }
    if (stream) (void)hipStreamDestroy(stream);
}

// The index lets go of its communicator — refused while a step made with it is still alive (the step's destructor and its queued merge
// refer to it); the sum hook that points into it goes first, so that a failed re-initialisation leaves no hook without a communicator.
static void comm_release(Index& idx, const char* who) {
    if (idx.comm && idx.comm->live != 0)
        throw VelociError(VQ_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(idx.comm->live) + " step(s) of this index are still in flight (vq_shard_step_end / vq_shard_step_free them first)");
    if (idx.allreduce_fn == comm_sum_u64) {
        idx.allreduce_fn = nullptr;
        idx.allreduce_ctx = nullptr;
    }
    idx.comm.reset();
}

int vq_comm_unique_id(void* id_out) {
    return guard([&] {
        if (!id_out) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_comm_unique_id: null argument");
        NcclId id;
        nccl_check(quiet_stdout([&] { return rccl_api().GetUniqueId(&id); }), "ncclGetUniqueId");
        std::memcpy(id_out, &id, sizeof id);
    });
}
int vq_comm_init(vq_index* index, int nranks, int rank, const void* unique_id) {
    return guard([&] {
        if (!index || !unique_id || nranks < 1 || rank < 0 || rank >= nranks) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_comm_init: bad argument");
        Index& idx = *index->idx;
        comm_release(idx, "vq_comm_init");
        VQ_HIP(hipSetDevice(idx.device));
        auto c = std::make_unique<ShardComm>();
        c->nranks = nranks;
        c->rank = rank;
        NcclId id;
        std::memcpy(&id, unique_id, sizeof id);
        ncclComm_t comm = nullptr;
        nccl_check(quiet_stdout([&] { return rccl_api().CommInitRank(&comm, nranks, id, rank); }), "ncclCommInitRank");
        c->nccl = comm;
        comm_setup(idx, std::move(c));
        idx.allreduce_fn = comm_sum_u64;
        idx.allreduce_ctx = &idx;
    });
}
int vq_comm_init_custom(vq_index* index, int nranks, int rank, vq_allgather_fn allgather, vq_allreduce_u32_fn allreduce_u32, void* ctx) {
    return guard([&] {
        if (!index || !allgather || nranks < 1 || rank < 0 || rank >= nranks) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_comm_init_custom: bad argument");
        auto c = std::make_unique<ShardComm>();
        c->nranks = nranks;
        c->rank = rank;
        c->allgather = allgather;
        c->allreduce_u32 = allreduce_u32;
        c->ctx = ctx;
        comm_release(*index->idx, "vq_comm_init_custom");
        comm_setup(*index->idx, std::move(c));
    });
}
int vq_comm_destroy(vq_index* index) {
    return guard([&] {
        if (!index) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_comm_destroy: null index");
        comm_release(*index->idx, "vq_comm_destroy");
    });
}

struct vq_shard_step {
    const Index* idx = nullptr;
    std::vector<std::unique_ptr<PartialBatch>> pbs;
    std::vector<size_t> first, arena_off;  // chunk c: its first request, the offset of its gathered copies inside the step's gather buffer
    size_t n = 0, used = 0;
    int parity = 0;
    bool merge_queued = false;
    bool counted = false;
    ~vq_shard_step() {
        pbs.clear();  // (the workspaces first: a parity is free once nothing of the step holds them)
        if (idx && idx->comm && idx->comm->unmerged == this) idx->comm->unmerged = nullptr;
        if (counted && idx && idx->comm) {
            idx->comm->live -= 1;
            idx->comm->busy[parity] = false;
        }
    }
};
namespace {
// A step failed as a whole on this rank (an exception between its collectives: out of device memory in a pre-pass, a failed launch), or did not
// complete in time: this rank's exchanges no longer line up with the other ranks'.  The communicator is marked down — every later step on it is
// refused — and an RCCL communicator is aborted, so that ranks waiting for this one inside a collective see an error instead of waiting for ever.
void comm_fail(ShardComm& c, const std::string& why) {
    if (!c.failed.empty()) return;
    c.failed = why;
    if (c.nccl) {
        try {
            if (rccl_api().CommAbort) (void)rccl_api().CommAbort(static_cast<ncclComm_t>(c.nccl));
            c.nccl = nullptr;  // (aborted: nothing is left to destroy)
        } catch (...) {
        }
    }
}
// Wait for a step's last event, but not for ever: a rank that never joined an exchange (it failed before, or died) must end this rank's step with
// an error, not hang it.  VQ_STEP_TIMEOUT_MS (default 120 000; 0: no limit).  An error RCCL reports asynchronously (a peer gone) ends the wait at once.
void bounded_wait(ShardComm& c, hipEvent_t ev) {
    static const long limit_ms = [] {
        const char* e = std::getenv("VQ_STEP_TIMEOUT_MS");
        return e ? std::atol(e) : 120000L;
    }();
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return;
        if (q != hipErrorNotReady) {
            comm_fail(c, std::string("the step's stream reported ") + hipGetErrorString(q));
            throw VelociError(VQ_ERR_DEVICE, "sharded step: " + c.failed);
        }
        if (spins < 2000) continue;  // (the usual case: the step is about to finish)
        if ((spins & 63u) == 0) {
            if (c.nccl && rccl_api().CommGetAsyncError) {
                int aerr = 0;
                if (rccl_api().CommGetAsyncError(static_cast<ncclComm_t>(c.nccl), &aerr) == 0 && aerr != 0) {
                    comm_fail(c, std::string("RCCL reported ") + (rccl_api().GetErrorString ? rccl_api().GetErrorString(aerr) : "an error") + " while the step was in flight (a rank is gone)");
                    throw VelociError(VQ_ERR_DEVICE, "sharded step: " + c.failed);
                }
            }
            const long waited = long(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count());
            if (limit_ms > 0 && waited > limit_ms) {
                comm_fail(c, "a step did not complete within " + std::to_string(limit_ms) + " ms (VQ_STEP_TIMEOUT_MS): a rank did not join its exchange");
                throw VelociError(VQ_ERR_DEVICE, "sharded step: " + c.failed);
            }
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}
// The scan stream of chunk k of a step.  Chunk 0: the index's.  Chunk 1 of an index that scans on its own stream: a second stream, so that the
// chunk's upload, memset, scans and span merge are not ordered behind chunk 0's — the second launch's workgroups take the wave slots the first
// one's tail leaves free, and chunk 0 of the NEXT step (behind chunk 0 of this one in stream order) does the same for this chunk's tail.  The
// chunks share nothing on the device: each has the workspace of its slot (upload area, span keys, partial, events).
// VQ_STEP_SCAN_STREAMS=1 (read once): every chunk on the index's scan stream.  A caller's stream (vq_index_set_stream/s) is never left.
hipStream_t step_scan_stream(const Index& idx, size_t k) {
    static const bool one = [] {
        const char* e = std::getenv("VQ_STEP_SCAN_STREAMS");
        return e && std::atoi(e) == 1;
    }();
    return k && !one && idx.stream == idx.own_stream && idx.own_stream2 ? idx.own_stream2 : idx.stream;
}
// Whether a step's scans are ordered behind the previous step's finalize and download (ev_fin).  On one scan stream they are: a scan launch fills
// every wave slot of the chip at once, and a finalize queued beside it waits for slots to free up (measured: 0.8-1.5 ms for a kernel that takes
// 8 us on an idle chip) — the GPU idles for the tens of microseconds of the exchange instead.  On two scan streams the wait would drain the chip
// at every step boundary, which is what the second stream is there to avoid: stream order alone keeps chunk k of a step behind chunk k of the
// step before.  VQ_STEP_FIN_WAIT=0 / 1 (read once) sets it for both cases.
bool step_waits_for_finalize(bool two_streams) {
    static const int knob = [] {
        const char* e = std::getenv("VQ_STEP_FIN_WAIT");
        return e ? int(std::atoi(e) != 0) : -1;
    }();
    return knob >= 0 ? knob != 0 : !two_streams;
}
// The step's finalize and download go onto the finish stream, behind its exchange and behind every chunk's scans and span merge (ev_done of the
// chunk's workspace, recorded on the chunk's own scan stream).  Whether the NEXT step's scans are ordered behind them: step_waits_for_finalize.
void step_queue_merge(vq_shard_step& step) {
    if (step.merge_queued) return;
    step.merge_queued = true;
    const Index& idx = *step.idx;
    ShardComm& c = *idx.comm;
    if (c.unmerged == &step) c.unmerged = nullptr;
    if (step.used) VQ_HIP(hipStreamWaitEvent(idx.fin_stream, c.ev_xchg[step.parity], 0));
    const uint8_t* gathered = static_cast<const uint8_t*>(c.gathered[step.parity].p);
    for (size_t k = 0; k < step.pbs.size(); ++k)
        finish_launch(idx, *step.pbs[k], step.used && step.pbs[k]->nq_dev ? gathered + step.arena_off[k] : nullptr, uint32_t(c.nranks));
    VQ_HIP(hipEventRecord(c.ev_fin[step.parity], idx.fin_stream));
}
}  // namespace

}  // extern "C"

// ---- the phases of vq_shard_step_begin, in the order it calls them
namespace {
// The index's communicator, up.  No communicator: the index is the only shard — the same pipeline without an exchange (two steps in flight on one GPU)
ShardComm& step_comm(const Index& idx) {
    if (!idx.comm) {
        auto local = std::make_unique<ShardComm>();
        comm_setup(const_cast<Index&>(idx), std::move(local));
    }
    ShardComm& c = *idx.comm;
    if (!c.failed.empty()) throw VelociError(VQ_ERR_DEVICE, "vq_shard_step_begin: the communicator is down (" + c.failed + "): make it again (vq_comm_init / vq_comm_init_custom) on every rank");
    return c;
}
// the step before this one: its merge goes out first, this step's scans are queued behind it
void step_queue_previous(const Index& idx, ShardComm& c, hipStream_t second) {
    if (!c.unmerged) return;
    vq_shard_step& prev = *c.unmerged;
    step_queue_merge(prev);
    const bool two_streams = second != idx.stream;
    if (step_waits_for_finalize(two_streams)) {
        VQ_HIP(hipStreamWaitEvent(idx.stream, c.ev_fin[prev.parity], 0));
        if (two_streams) VQ_HIP(hipStreamWaitEvent(second, c.ev_fin[prev.parity], 0));
    }
}
std::unique_ptr<vq_shard_step> step_claim_parity(const Index& idx, ShardComm& c, size_t n) {
    if (c.live >= 2) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_shard_step_begin: two steps are in flight already (end one first)");
    auto step = std::make_unique<vq_shard_step>();
    step->idx = &idx;
    step->counted = true;
    c.live += 1;
    step->n = n;
    // the parity (workspace pair, gather buffer, events) no live step holds — not a running count: steps may end in any order, and a
    // begin that throws (a pre-pass out of memory) is retried while the other step is still in flight
    step->parity = c.busy[0] ? 1 : 0;
    if (c.busy[step->parity]) {
        step->counted = false;
        c.live -= 1;
        throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_shard_step_begin: both step slots are held (end a step first)");
    }
    c.busy[step->parity] = true;
    return step;
}
// compile + scans.  Every chunk shares its requests with their handles (keep_requests): the handles may go before the step ends
void step_run_chunks(vq_shard_step& step, const vq_request* const* requests, const std::vector<const Request*>& reqs, hipStream_t second) {
    const Index& idx = *step.idx;
    const size_t n = step.n;
    // One launch per step: with two steps in flight the compilation of step i + 1 already overlaps the scans of step i, and one launch of
    // 1024 requests fills the chip more evenly than two of 512 (100 M docs: 7.25 against 7.41 ms per step).  VQ_SHARD_CHUNKS=2 cuts a step in two.
    // (read at every step: a host program may cut only some of its steps in two — bench.py does for the headline's launches of distinct queries)
    const size_t chunks_env = [] {
        const char* e = std::getenv("VQ_SHARD_CHUNKS");
        return size_t(e ? std::min(2, std::max(1, std::atoi(e))) : 0);
    }();
    const size_t nchunks = chunks_env && n >= 512 ? chunks_env : 1;
    for (size_t k = 0; k < nchunks; ++k) {
        const size_t b = n * k / nchunks, e = n * (k + 1) / nchunks;
        step.first.push_back(b);
        step.pbs.push_back(run_partial(idx, reqs.data() + b, e - b, step.parity * 2 + int(k), -1, k ? second : idx.stream));
        keep_requests(*step.pbs.back(), requests + b, e - b);
    }
}
// The exchange: behind the step's scans, on the collective stream.  Per chunk the part of its partial in front of the histograms
// (hit counts, statistics, top-k keys: the same size on every rank) is all-gathered, the histograms are summed in place.
void step_queue_exchange(vq_shard_step& step, bool exchange) {
    const Index& idx = *step.idx;
    ShardComm& c = *idx.comm;
    size_t off = 0;
    for (auto& pb : step.pbs) {
        step.arena_off.push_back(off);
        if (exchange && pb->nq_dev) off += (size_t(pb->layout.off_hist) * size_t(c.nranks) + 255) / 256 * 256;
    }
    step.used = off;
    if (!off) return;
    VQ_HIP(hipEventRecord(c.ev_scan[step.parity], idx.stream));
    VQ_HIP(hipStreamWaitEvent(c.stream, c.ev_scan[step.parity], 0));
    c.gathered[step.parity].ensure(off);
    uint8_t* gathered = c.gathered[step.parity].as<uint8_t>();
    for (size_t k = 0; k < step.pbs.size(); ++k) {
        PartialBatch& pb = *step.pbs[k];
        if (!pb.nq_dev) continue;
        const size_t bytes = size_t(pb.layout.off_hist);
        if (c.nccl) nccl_check(rccl_api().AllGather(pb.d_partial, gathered + step.arena_off[k], bytes, kNcclUint8, static_cast<ncclComm_t>(c.nccl), c.stream), "ncclAllGather");
        else if (c.allgather(c.ctx, pb.d_partial, gathered + step.arena_off[k], bytes, c.stream) != 0) throw VelociError(VQ_ERR_DEVICE, "sharded step: the caller's all-gather failed");
        if (pb.layout.total_hist) {  // facet counts are additive: summed in place, read by this rank's merge
            void* h = pb.d_partial + pb.layout.off_hist;
            if (c.nccl) nccl_check(rccl_api().AllReduce(h, h, size_t(pb.layout.total_hist), kNcclUint32, kNcclSum, static_cast<ncclComm_t>(c.nccl), c.stream), "ncclAllReduce");
            else if (!c.allreduce_u32 || c.allreduce_u32(c.ctx, h, size_t(pb.layout.total_hist), c.stream) != 0)
                throw VelociError(VQ_ERR_DEVICE, "sharded step: the caller's all-reduce failed");
        }
    }
    VQ_HIP(hipEventRecord(c.ev_xchg[step.parity], c.stream));
}
}  // namespace

extern "C" {

int vq_shard_step_begin(const vq_index* index, const vq_request* const* requests, size_t n, vq_shard_step** out) {
    return guard([&] {
        if (!index || !out || (n && !requests)) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_shard_step_begin: null argument");
        *out = nullptr;
        const Index& idx = *index->idx;
        ShardComm& c = step_comm(idx);
        const bool exchange = c.nccl != nullptr || c.allgather != nullptr;
        static const bool timing = std::getenv("VQ_TIMING") != nullptr;
        const auto tb0 = std::chrono::steady_clock::now();
        VQ_HIP(hipSetDevice(idx.device));
        const std::vector<const Request*> reqs = request_pointers(requests, n);
        // An index that answers alone, on its own streams: the second chunk of a step goes onto a scan stream of its own (step_scan_stream), and
        // the step does not wait for the previous step's finalize (step_queue_merge).  With an exchange the step stays on one scan stream.
        const hipStream_t second = exchange ? idx.stream : step_scan_stream(idx, 1);
        step_queue_previous(idx, c, second);
        const auto tb1 = std::chrono::steady_clock::now();
        std::unique_ptr<vq_shard_step> step = step_claim_parity(idx, c, n);
        auto tb2 = tb1;
        try {
            step_run_chunks(*step, requests, reqs, second);
            tb2 = std::chrono::steady_clock::now();
            step_queue_exchange(*step, exchange);
        } catch (const std::exception& ex) {
            // Whatever was thrown from here on ends the step on THIS rank only (requests that fail on their own ride along as statuses and never
            // throw): with other ranks around, their exchange of this step will miss this rank — the communicator goes down with the step.
            if (exchange && c.nranks > 1) comm_fail(c, std::string("a step failed on rank ") + std::to_string(c.rank) + ": " + ex.what());
            throw;
        }
        c.unmerged = step.get();
        *out = step.release();
        if (timing) {
            const auto tb3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::fprintf(stderr, "[vq timing] shard step begin %.3f ms (queue the previous merge %.3f, compile + scans %.3f, exchange calls %.3f)\n", ms(tb0, tb3), ms(tb0, tb1), ms(tb1, tb2), ms(tb2, tb3));
        }
    });
}

int vq_shard_step_end(vq_shard_step* step_raw, size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status) {
    std::unique_ptr<vq_shard_step> step(step_raw);  // freed whatever happens
    return guard([&] {
        if (!step || (step->n && (!num_hits || !counts || !ids || !scores))) throw VelociError(VQ_ERR_INVALID_ARGUMENT, "vq_shard_step_end: null argument");
        const Index& idx = *step->idx;
        ShardComm& c = *idx.comm;
        VQ_HIP(hipSetDevice(idx.device));
        static const bool timing = std::getenv("VQ_TIMING") != nullptr;
        const auto te0 = std::chrono::steady_clock::now();
        if (!c.failed.empty()) throw VelociError(VQ_ERR_DEVICE, "vq_shard_step_end: the communicator is down (" + c.failed + ")");
        step_queue_merge(*step);
        bounded_wait(c, c.ev_fin[step->parity]);
        if (timing) {
            VQ_HIP(hipStreamSynchronize(idx.fin_stream));
            std::fprintf(stderr, "[vq timing] shard step end: waited %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te0).count());
        }
        const uint8_t* gathered = static_cast<const uint8_t*>(c.gathered[step->parity].p);
        for (size_t k = 0; k < step->pbs.size(); ++k) {
            std::vector<std::unique_ptr<Result>> results;
            std::vector<int> st;
            std::vector<std::string> errs;
            finish_batch(idx, *step->pbs[k], step->used && step->pbs[k]->nq_dev ? gathered + step->arena_off[k] : nullptr, uint32_t(c.nranks), results, st, errs);
            // a request that reaches beyond one scan's ranking: on an index that answers alone (no exchange) its further pages are scanned here, like on
            // the flat batch path; over shards every rank would have to page on the MERGED page — declined there (vq_merge_partials pages)
            if (!step->used && c.nranks == 1) complete_deep_requests(idx, step->pbs[k]->reqs.data(), step->pbs[k]->reqs.size(), results, st, errs);
            else decline_deep(results, st, errs);
            decline_explain(results, st, errs, "the sharded step");
            copy_flat(results, st, errs, step->first[k], stride, num_hits, counts, ids, scores, status);
            step->pbs[k].reset();  // (destroyed here, by the thread that uses these allocations next: handing the frees to a background thread was tried and
                                   //  cost more than it saved — it frees into the arenas the compile threads are allocating from)
        }
        if (timing) std::fprintf(stderr, "[vq timing] shard step end total %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te0).count());
    });
}
void vq_shard_step_free(vq_shard_step* step) { delete step; }

int vq_shard_step_flat(const vq_index* index, const vq_request* const* requests, size_t n, size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids,
                       float* scores, int* status) {
    vq_shard_step* step = nullptr;
    const int rc = vq_shard_step_begin(index, requests, n, &step);
    if (rc != VQ_OK) return rc;
    return vq_shard_step_end(step, stride, num_hits, counts, ids, scores, status);
}

}  // extern "C"
