// vgan soibean over the device front end's pipeline (reference: src/getLCAfromGAM.h:31-45 -- analyse_GAM's loop over the
// stream -- feeding the per-read body of :92-186): the consumer of csrc/gam_pipe.hip's pieces for soibean.  A piece's reads go through
// soibean's flatten as kernels (sb_flatten_kernels.hip) into the batch of the lane's context, which grows in HBM piece by piece; the
// reads the device flatten leaves (indels, soft clips, anything the reference would index out of bounds on) go through the host's parser
// and vgan_sb_flatten behind the slot's back and are appended at the end; then analyse_GAM's tables are made ONCE per context over its
// whole batch (vgan_sb_precompute).  Which context a read lands in and where in its batch does not change a bit of what the chains
// compute: their sums over reads are integers (csrc/sb_device.h: SbFix), the signature counts are counts.  No kernel lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gam_device.h"
#include "gam_object.h"
#include "host/common.h"
#include "sb_device.h"
#include "vgan_gpu.h"

using namespace vgan;
using namespace vgan::gd;

namespace {
struct SbLeftJob : GamJob { // the reads of one piece that the device flatten leaves to the host
    int lane = 0;
    int64_t piece = 0;
    LeftReads left;
    vgan_sb_host_batch *hb = nullptr;
    vgan_sb_flatten_stats st{};
    ~SbLeftJob() { vgan_sb_host_batch_free(hb); }
};
} // namespace

struct vgan_sb_gamrun : GamRun<vgan_sb_ctx, vgan_sb_devflat, SbLeftJob> {
    bool finished = false;
    vgan_sb_gam_result res{};
    double ms_tables = 0;

    int consume(int lane, vgan_gamdev *g, uint64_t read_base, const uint8_t *, int64_t piece) override {
        const int64_t R = piece_reads(g, read_base);
        if (R < 0) return (int)R;
        std::vector<uint8_t> mask((size_t)R, 0);
        int r;
        {
            std::lock_guard<std::mutex> lk(lane_mu[(size_t)lane]); // (the lane's batch and its stream: one piece at a time)
            const size_t l = (size_t)lane;
            if (!df[l]) {
                if ((r = vgan_sb_devflat_create(ctx[l], graph, &df[l])) < 0) return r;
                // the lane's share of the input over this piece: the batch's arrays are sized once
                const double pieces = (double)n / (double)std::max<uint64_t>(opts.piece_bytes, 1) / (double)devices.size();
                (void)vgan_sb_devflat_expect(df[l], std::max(1.0, pieces * 1.1 + 0.5));
            }
            vgan_sb_flatten_stats st{};
            if ((r = vgan_sb_devflat_append_gamdev(df[l], g, (uint32_t)read_base, mask.data(), &st)) < 0) return r;
            std::lock_guard<std::mutex> lk2(mu);
            n_device_reads += (uint64_t)st.n_out;
        }
        auto job = std::make_shared<SbLeftJob>();
        if ((r = job->left.pick(g, mask.data(), (uint64_t)R, read_base, tool)) < 0 || job->left.where.empty()) return r;
        job->lane = lane;
        job->piece = piece;
        vgan_sb_gamrun *self = this;
        job->t = std::thread([self, job] {
            vgan_alnset merged;
            if ((job->rc = job->left.parse(self->host_threads, self->tool, merged)) >= 0)
                job->rc = vgan_sb_flatten(self->graph, &merged, 0, merged.n_reads(), self->host_threads, &job->hb, &job->st);
            if (job->rc < 0) job->err = last_error();
        });
        std::lock_guard<std::mutex> lk(mu);
        bg.push_back(job);
        n_host_reads += job->left.where.size();
        return VGAN_OK;
    }
};

extern "C" int vgan_sb_gam_start(const int *devices, int n_lanes, const void *bytes, uint64_t n, const vgan_gampipe_opts *opts, vgan_sb_gamrun **out) {
    return gamrun_start("sb", devices, n_lanes, bytes, n, opts, out, [](vgan_sb_gamrun &r) {
        r.opts.keep_unmapped = 0;   // getLCAfromGAM.h:101: identity == 0 is skipped
        r.opts.mark_duplicates = 0; // (soibean removes no duplicates)
    });
}

extern "C" int vgan_sb_gam_attach(vgan_sb_gamrun *r, vgan_sb_ctx *const *ctxs, int n_ctx, const vgan_graph *graph) {
    return gamrun_attach("sb", r, ctxs, n_ctx, graph);
}

extern "C" int vgan_sb_gam_finish(vgan_sb_gamrun *r, vgan_sb_gam_result *res, vgan_gampipe_stats *pstats) {
    if (!r) return fail(VGAN_EINVAL, "vgan_sb_gam_finish: null argument");
    if (res) memset(res, 0, sizeof *res);
    r->join();
    if (r->rc >= 0 && !r->finished) {
        r->finished = true;
        const auto t0 = std::chrono::steady_clock::now();
        // the host's batches behind the device's, in the order of the pieces (any order gives the same tables' sums; this one is repeatable)
        std::stable_sort(r->bg.begin(), r->bg.end(), [](const std::shared_ptr<SbLeftJob> &a, const std::shared_ptr<SbLeftJob> &b) { return a->piece < b->piece; });
        for (auto &j : r->bg) {
            const size_t l = (size_t)j->lane;
            vgan_sb_batch hb;
            int rc = vgan_sb_host_batch_get(j->hb, &hb);
            if (rc >= 0 && hb.n_reads && !r->df[l]) rc = vgan_sb_devflat_create(r->ctx[l], r->graph, &r->df[l]);
            if (rc >= 0) rc = vgan_sb_devflat_append_host(r->df[l], &hb, j->left.where.data());
            if (rc < 0) {
                r->rc = rc;
                r->err = last_error();
                break;
            }
            r->res.n_bad += j->st.n_bad;
            vgan_sb_host_batch_free(j->hb);
            j->hb = nullptr;
        }
        for (size_t l = 0; l < r->ctx.size() && r->rc >= 0; ++l) { // analyse_GAM's tables, once per context (an empty share gives empty tables)
            vgan_sb_batch b{};
            int64_t bad = 0;
            int rc = r->df[l] ? vgan_sb_devflat_batch(r->df[l], &b) : VGAN_OK;
            if (rc >= 0) rc = vgan_sb_precompute(r->ctx[l], &b, &bad);
            if (rc < 0) {
                r->rc = rc;
                r->err = last_error();
                break;
            }
            r->res.n_dev_bad += bad;
            r->res.n_reads += b.n_reads;
        }
        r->ms_tables = ms_since(t0);
        for (size_t l = 0; l < r->df.size(); ++l) r->pst.device_bytes += sb_devflat_device_bytes(r->df[l]);
    }
    if (pstats) *pstats = r->pst;
    if (r->rc < 0) return fail(r->rc, "%s", r->err.c_str());
    r->res.n_messages = (int64_t)r->pst.n_messages;
    r->res.n_mapped = (int64_t)r->pst.n_reads;
    r->res.ms_tables = r->ms_tables;
    if (res) *res = r->res;
    return VGAN_OK;
}

// the batch of lane `lane` as the tables were made from it (device pointers; valid until vgan_sb_gam_free): read_src = the reads' places
// among the file's mapped reads
extern "C" int vgan_sb_gam_batch(const vgan_sb_gamrun *r, int lane, vgan_sb_batch *out) {
    if (!r || !out || lane < 0 || lane >= (int)r->df.size()) return fail(VGAN_EINVAL, "vgan_sb_gam_batch: bad argument");
    if (!r->finished) return fail(VGAN_ESTATE, "vgan_sb_gam_batch: the run has not finished");
    if (!r->df[(size_t)lane]) {
        memset(out, 0, sizeof *out);
        out->on_device = 1;
        return VGAN_OK;
    }
    return vgan_sb_devflat_batch(r->df[(size_t)lane], out);
}

extern "C" void vgan_sb_gam_free(vgan_sb_gamrun *r) {
    if (!r) return;
    if (r->coord.joinable()) {
        r->finished = true; // (no tables for a run that is thrown away)
        (void)vgan_sb_gam_finish(r, nullptr, nullptr);
    }
    r->bg.clear();
    for (auto *f : r->df) vgan_sb_devflat_free(f);
    delete r;
}
