// sharded.hip -- one frame over several GPUs: the communicator (comm.cpp)
// and nori_gpu_render_sharded, this rank's share (shard.cpp) through render().
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ctx.h"

extern "C" {

int nori_gpu_comm_id(unsigned char *id) {
    return guarded([&] {
        if (!id) return fail(NORI_ERR_INVALID, "null argument");
        comm_unique_id(id);
        return (int)NORI_OK;
    });
}
int nori_gpu_comm_create(const unsigned char *id, int nranks, int rank, int device, nori_gpu_comm **out) {
    return guarded([&] {
        if (!id || !out) return fail(NORI_ERR_INVALID, "null argument");
        if (nranks < 1 || nranks > 0xFFFF || rank < 0 || rank >= nranks) return fail(NORI_ERR_INVALID, "rank out of range");
        std::unique_ptr<nori_gpu_comm> c(new nori_gpu_comm);
        // the status exchange's words, allocated here so that no allocation
        // stands between a failed share and the exchange
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc((void **)&c->status_dev, sizeof(int)));
        HIP_TRY(hipHostMalloc((void **)&c->status_host, sizeof(int), hipHostMallocDefault));
        c->nccl = comm_create(id, nranks, rank, device);
        c->nranks = nranks;
        c->rank = rank;
        c->device = device;
        *out = c.release();
        return (int)NORI_OK;
    });
}
int nori_gpu_comm_rank(const nori_gpu_comm *c, int *nranks, int *rank) {
    if (!c || !nranks || !rank) return fail(NORI_ERR_INVALID, "null argument");
    *nranks = c->nranks;
    *rank = c->rank;
    return NORI_OK;
}
void nori_gpu_comm_destroy(nori_gpu_comm *c) { delete c; }
const char *nori_gpu_comm_library(void) { return comm_library_path(); }

int nori_gpu_render_sharded(nori_gpu_ctx *c, nori_gpu_comm *comm, const nori_gpu_render_desc *rd, int mode, int root,
                            float *film, nori_gpu_stats *stats) {
    return guarded([&] {
        if (!c || !comm) return fail(NORI_ERR_INVALID, "null argument");
        if (comm->aborted) return fail(NORI_ERR_HIP, "communicator was aborted by an earlier failure");
        // This rank's share.  A failure or a cancel (nori_gpu_cancel) must not
        // leave the peers blocked in the film sum: every rank joins a status
        // exchange first (max over ranks of severity << 16 | rank), and the
        // film sum runs only if every rank rendered its share.  Everything
        // fallible of the share -- argument checks, the film clear, the
        // render -- reports through the exchange.
        int rc = NORI_OK;
        std::string err;
        double own_s = 0.0, own_samples = 0.0, max_samples = 0.0;
        size_t n = 0;
        try {
            if (!rd || !film) throw NoriException(NORI_ERR_INVALID, "null argument");
            if (rd->num_blocks && !rd->block_ids) throw NoriException(NORI_ERR_INVALID, "block_ids is null");
            if (rd->variance_out)  // per-pixel statistics are not summed across ranks
                throw NoriException(NORI_ERR_INVALID, "nori_gpu_render_sharded: variance_out must be NULL");
            if (root >= comm->nranks) throw NoriException(NORI_ERR_INVALID, "root out of range");
            if (comm->device != c->device)
                throw NoriException(NORI_ERR_INVALID, "communicator and context on different devices");
            HIP_TRY(hipSetDevice(c->device));
            std::vector<uint32_t> blocks, other;
            nori_gpu_render_desc s = shard_of(c->S.W, c->S.H, c->spp, *rd, mode, comm->nranks, comm->rank, blocks);
            own_samples = share_samples(c->S.W, c->S.H, s);
            for (int r = 0; r < comm->nranks; ++r)
                max_samples = std::max(max_samples, share_samples(c->S.W, c->S.H,
                                                                  shard_of(c->S.W, c->S.H, c->spp, *rd, mode,
                                                                           comm->nranks, r, other)));
            s.output_on_device = 1;
            s.variance_out = nullptr;
            n = 4 * (size_t)(c->S.W + 2 * c->S.border) * (size_t)(c->S.H + 2 * c->S.border);
            HIP_TRY(hipMemsetAsync(film, 0, n * sizeof(float), c->stream));
            const auto t0 = std::chrono::steady_clock::now();
            if (s.pass_count) rc = render(*c, s, film, stats);
            else if (stats) std::memset(stats, 0, sizeof(*stats));
            own_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        } catch (const NoriException &e) {
            rc = e.code;
            err = e.what();
        } catch (const std::bad_alloc &) {
            rc = NORI_ERR_OOM;
            err = "out of memory";
        } catch (const std::exception &e) {
            rc = NORI_ERR_INVALID;
            err = e.what();
        }
        if (rc != NORI_OK && err.empty()) err = last_error();
        if (rc == NORI_ERR_HIP) {
            // A sticky error (a device fault) fails every later call on the
            // device, so this rank cannot join the exchange: abort, and the
            // peers' watchdog ends their wait.  Any other HIP error leaves
            // the stream usable and goes through the exchange.
            (void)hipGetLastError();
            if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
                comm_abort(comm->nccl);
                comm->aborted = true;
                return fail(rc, err);
            }
        }
        const double timeout = comm_timeout_s(rc, own_s, own_samples, max_samples);
        const int all = comm_max_int(comm->nccl, comm->status_dev, comm->status_host,
                                     comm_status_word(rc, comm->rank), c->stream, timeout, comm->aborted);
        if (rc != NORI_OK) return fail(rc, err);
        if ((all >> 16) != 0)
            return fail((all >> 16) == 1 ? NORI_ERR_CANCELLED : NORI_ERR_INVALID,
                        "the frame is incomplete: rank " + std::to_string(all & 0xFFFF) +
                            ((all >> 16) == 1 ? " was cancelled" : " failed to render its share"));
        comm_sum(comm->nccl, film, n, root, c->stream);
        comm_wait(comm->nccl, c->stream, timeout, comm->aborted);
        return (int)NORI_OK;
    });
}

}  // extern "C"
