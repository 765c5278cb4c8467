// What capi.cpp, capi_debug.cpp and shard_step.cpp share and nobody else needs: the handles behind include/veloci_amd.h, the error text and the
// guard of the ABI, and the helpers between a batch of request handles and the flat outputs.  Each is defined once (capi.cpp).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/veloci_amd.h"
#include "engine.hpp"

struct vq_index_builder {
    vq::IndexBuilder b;
};
struct vq_index {
    std::unique_ptr<vq::Index> idx;
};
// Shared with every batch that a caller holds (PartialBatch::owners): the handle may be freed, or given another doc set, while such a batch or
// step is alive.  vq_request_set_docset copies the request first when a batch shares it.
struct vq_request {
    std::shared_ptr<vqreq::Request> req;
};
struct vq_docset {
    std::shared_ptr<const vq::DocSet> set;
};
struct vq_result {
    vq::Result r;
};
struct vq_docset_aggs {
    std::vector<vq::AggResult> r;  // the buckets the C structs point into
    std::vector<vq_docset_agg> c;
};
struct vq_docset_top {
    vq::TopResult r;
};
struct vq_partial_batch {
    std::unique_ptr<vq::PartialBatch> pb;
};
struct vq_suggest_result {
    std::vector<vq::SuggestEntry> e;
};

namespace vq {
extern thread_local std::string g_err;  // vq_last_error

int fail(int code, const std::string& msg);
template <class F>
int guard(F f) {
    try {
        f();
        g_err.clear();
        return VQ_OK;
    } catch (const vqreq::VelociError& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(VQ_ERR_DEVICE, "out of host memory");
    } catch (const std::exception& e) {
        return fail(VQ_ERR_INVALID_ARGUMENT, e.what());
    }
}

// the requests behind the handles of a batch (a null handle stays null: that request alone fails)
std::vector<const vqreq::Request*> request_pointers(const vq_request* const* requests, size_t n);
// a batch that outlives the call that made it shares its requests with their handles from here on
void keep_requests(PartialBatch& pb, const vq_request* const* requests, size_t n);
void decline_deep(std::vector<std::unique_ptr<Result>>& results, std::vector<int>& st, std::vector<std::string>& errs);
void decline_explain(std::vector<std::unique_ptr<Result>>& results, std::vector<int>& st, std::vector<std::string>& errs, const char* where);
void copy_flat(const std::vector<std::unique_ptr<Result>>& results, const std::vector<int>& st, const std::vector<std::string>& errs, size_t base,
               size_t stride, uint64_t* num_hits, uint32_t* counts, uint32_t* ids, float* scores, int* status);
}  // namespace vq
