// The GAM front end's device object (gam_kernels.hip makes and fills it; gam_pipe.hip runs several of them as a pipeline over the
// file's pieces).  Private to the library: the C-ABI sees an opaque vgan_gamdev.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gam_device.h"
#include "host/common.h"
#include "vgan_gpu.h"

namespace vgan {
namespace gd {

enum : uint32_t { GD_OK = 0, GD_BAD_BLOCK = 1, GD_BAD_CODE = 2, GD_OVERRUN_IN = 3, GD_OVERRUN_OUT = 4, GD_BAD_STORED = 5, GD_BAD_CRC = 6, GD_PUNT = 7 /* gd_tokens_kernel leaves the member to gd_inflate_kernel */ };
enum : uint32_t { GF_OK = 0, GF_BAD_VARINT = 1, GF_MISSED = 2, GF_TRUNCATED = 3, GF_BAD_MESSAGE = 4 };

struct GdMapRec { // what the message pass leaves per mapping for the lane that fills its arrays
    uint64_t pos;   // the mapping's bytes: offset in the inflated stream | length << 40
    uint32_t e_at;  // its first edit's index
    uint32_t s_at;  // its first edit-sequence byte's index
};
static_assert(sizeof(GdMapRec) == 16, "one 16-byte store per mapping");

// Where a piece's framing walk stood when the piece's bytes ended (libvgio's stream: groups {count, count x (length, bytes)}): the
// bytes from `p` on -- an item the piece holds the beginning of -- go in front of the next piece's inflated bytes, whose walk takes up
// the state.  mode 0: before a group's count; 1: inside a group, `rem` items to go (`first`: the next one may be the group's tag);
// 2: inside a group whose count the walk never saw (it started from a tag found in the bytes: that group ends where a count is followed by
// a tag).
struct GdCarryState {
    uint64_t p, rem;
    uint32_t mode, first;
};
struct GdCarry {
    GdCarryState st{0, 0, 0, 0};
    std::vector<uint8_t> tail; // the stream's bytes from st.p on (host)
};

extern double g_alloc_ms; // (VGAN_TIMING: what hipMalloc took, summed)
template <class T> struct GBuf {
    T *p = nullptr;
    size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap && p) return VGAN_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const auto t_alloc = std::chrono::steady_clock::now();
        struct Acc {
            std::chrono::steady_clock::time_point t0;
            ~Acc() { g_alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
        } acc{t_alloc};
        const size_t want = n + std::min<size_t>(n / 8, ((size_t)16 << 20) / sizeof(T)) + 64;
        const hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? VGAN_ENOMEM : VGAN_ENODEV, "the GAM front end on the device: hipMalloc of %zu bytes failed: %s", want * sizeof(T),
                        hipGetErrorString(e));
        }
        cap = want;
        // (test aid: fresh device memory is often zero in a young process and someone's old data in an old one -- a kernel that leaves
        // an entry unwritten passes every test but the one that runs late)
        static const bool poison = getenv("VGAN_POISON_ALLOCS") != nullptr;
        if (poison) {
            if (hipMemset(p, 0xA5, want * sizeof(T)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) // (the fill runs on the null stream, the kernels on others)
                return fail(VGAN_ENODEV, "the GAM front end on the device: hipMemset failed");
        }
        return VGAN_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The (node id, offset) keys of the first mappings seen so far, in ascending order (signed, node first): what makes a read of a later
// piece a duplicate of a read of an earlier one (src/rmdup.cpp keeps the FIRST read of a key).  One per pipeline lane, on its device.
struct GdSeen {
    GBuf<int64_t> node[2], off[2];
    int cur = 0;
    uint64_t n = 0;
    size_t merged = 0; // how many of the pipeline's key lists (one per piece, kept on the host) this set holds
    void release() {
        for (int k = 0; k < 2; ++k) node[k].release(), off[k].release();
        n = 0;
    }
};
struct GdKeyList { // the keys a piece added (host copy: the other lanes' sets take them up)
    int lane = -1;
    std::vector<int64_t> node, off;
};

} // namespace gd
} // namespace vgan

#ifndef GD_PIECES_N
#define GD_PIECES_N 4
#endif

struct vgan_gamdev {
    static constexpr int GD_PIECES = GD_PIECES_N;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    vgan::gd::GBuf<uint8_t> in, infl, cub_tmp;
    vgan::gd::GBuf<vgan::GdBlock> blocks;
    vgan::gd::GBuf<uint32_t> status, seg_msgs, seg_status, msg_len, keep, n_map, n_edit, n_eseq, n_qual, r_at, m_at, e_at, s_at, q_at, bad;
    vgan::gd::GBuf<uint64_t> anchor, next_anchor, msg_base, msg_off;
    vgan::gd::GBuf<vgan::gd::GdCarryState> carry;
    vgan::gd::GBuf<uint64_t> tok_reg;              // gd_tokens_kernel -> gd_lz_kernel: {first token, tokens} per block of a member (the tokens themselves borrow map_rec)
    vgan::gd::GBuf<uint32_t> tok_nreg, tok_cursor; // blocks per member; the scratch's fill
    vgan::gd::GBuf<uint32_t> crc_want, crc_tab;    // the members' CRC-32 as their trailers say; gd_crc_kernel's tables
    std::vector<uint32_t> h_crc;                   // (host copy of crc_want: the members the older kernel does again are checked again)
    vgan::gd::GBuf<vgan::gd::GdMapRec> map_rec; // per mapping: where its bytes lie, where its edits go (gd_fill_kernel -> gd_fill_maps_kernel)
    // one DfSlice's arrays (hc_flatten_kernels.hip) of the file's reads
    vgan::gd::GBuf<uint32_t> map_off, qual_off, edit_off, e_seq_off, m_node, seq_len;
    vgan::gd::GBuf<int32_t> m_offset, mapq, e_len;
    vgan::gd::GBuf<uint8_t> unmapped, m_rev, e_seq, qual;
    vgan::gd::GBuf<int64_t> first_node, first_offset;
    vgan::gd::GBuf<uint8_t> dup, picked_bytes;           // duplicate marks per read; the messages handed back to the host
    vgan::gd::GBuf<uint64_t> sort_key, sort_key2, picked_off;
    vgan::gd::GBuf<uint32_t> perm_a, perm_b, new_flag, new_at;
    vgan::gd::GBuf<int64_t> new_node, new_off;
    hipStream_t piece_stream[GD_PIECES] = {}; // the file's (or a piece's) bytes go up in a few parts, each copied and inflated on a stream of its own
    // the stream the framing and the parse read: `u` = infl.p + tail_cap - (bytes carried over from the piece before), n_stream bytes
    uint64_t tail_cap = 0;
    const uint8_t *u = nullptr;
    uint64_t n_stream = 0;
    size_t n_blocks = 0;
    uint64_t n_redone = 0;     // (test aid) members the two-kernel inflate left to the older kernel
    bool inflate_checked = false; // gd_piece_inflated has waited for this piece's inflate and looked at its members' states
    uint64_t n_reanchored = 0; // (test aid) tag-like bytes the framing of the parses so far took for a group's tag and gave up again
    uint64_t n_picked = 0, n_picked_bytes = 0;
    uint64_t n_inflated = 0, n_messages = 0, R = 0, M = 0, E = 0, S = 0, Q = 0;
    double ms_inflate = 0, ms_frame = 0, ms_parse = 0, ms_upload = 0;
    size_t device_bytes() const { // what the object holds of the device's memory
        size_t b = in.cap + infl.cap + cub_tmp.cap + blocks.cap * sizeof(vgan::GdBlock) + carry.cap * sizeof(vgan::gd::GdCarryState) + map_rec.cap * sizeof(vgan::gd::GdMapRec);
        for (auto *x : {&status, &seg_msgs, &seg_status, &msg_len, &keep, &n_map, &n_edit, &n_eseq, &n_qual, &r_at, &m_at, &e_at, &s_at, &q_at, &bad, &map_off, &qual_off,
                        &edit_off, &e_seq_off, &m_node, &seq_len, &perm_a, &perm_b, &new_flag, &new_at})
            b += x->cap * 4;
        for (auto *x : {&anchor, &next_anchor, &msg_base, &msg_off, &sort_key, &sort_key2, &picked_off, &tok_reg}) b += x->cap * 8;
        b += (tok_nreg.cap + tok_cursor.cap + crc_want.cap + crc_tab.cap) * 4;
        for (auto *x : {&m_offset, &mapq, &e_len}) b += x->cap * 4;
        for (auto *x : {&unmapped, &m_rev, &e_seq, &qual, &dup, &picked_bytes}) b += x->cap;
        for (auto *x : {&first_node, &first_offset, &new_node, &new_off}) b += x->cap * 8;
        return b;
    }
    void release_all() {
        in.release(), infl.release(), cub_tmp.release(), blocks.release();
        for (auto *b : {&status, &seg_msgs, &seg_status, &msg_len, &keep, &n_map, &n_edit, &n_eseq, &n_qual, &r_at, &m_at, &e_at, &s_at, &q_at, &bad, &map_off,
                        &qual_off, &edit_off, &e_seq_off, &m_node, &seq_len})
            b->release();
        for (auto *b : {&anchor, &next_anchor, &msg_base, &msg_off}) b->release();
        carry.release();
        tok_reg.release(), tok_nreg.release(), tok_cursor.release(), crc_want.release(), crc_tab.release();
        map_rec.release();
        for (auto *b : {&m_offset, &mapq, &e_len}) b->release();
        for (auto *b : {&unmapped, &m_rev, &e_seq, &qual}) b->release();
        first_node.release(), first_offset.release();
        dup.release(), picked_bytes.release(), sort_key.release(), sort_key2.release(), picked_off.release();
        for (auto *b : {&perm_a, &perm_b, &new_flag, &new_at}) b->release();
        new_node.release(), new_off.release();
    }
};

namespace vgan {
namespace gd {
// ---- a file in pieces (gam_kernels.hip): what vgan_gamdev_parse does in one go, cut at BGZF member boundaries
// The piece's bytes go up and its members are inflated behind them (asynchronous: gd_piece_parse waits).  blocks: the piece's members,
// in_off relative to `bytes`, out_off relative to the piece's first inflated byte; tail_cap: room kept in front of the inflated bytes
// for what the piece before leaves over; crcs: the members' CRC-32 as their trailers say (checked on the device: GD_BAD_CRC).
int gd_piece_upload_inflate(vgan_gamdev *g, const uint8_t *bytes, uint64_t n_bytes, const GdBlock *blocks, const uint32_t *crcs, size_t n_blocks, uint64_t total_out,
                            uint64_t tail_cap);
// Framing from the state `in` (its tail in front of the inflated bytes) + the protobuf walk: the piece's arrays as vgan_gamdev_parse
// leaves a file's.  `last`: the stream ends with this piece (a walk that ends inside an item is then a truncated file); otherwise `out`
// takes the state and the bytes left over.  frame_done (or null) is called once `out` is final: the next piece's framing may start then.
// Waits for the piece's inflate and checks its members (a member the two kernels left is done again by the older one; a wrong CRC-32 is an
// error).  Needs nothing of the piece before: a caller makes it BEFORE it takes its turn at the framing's hand-over (gd_piece_parse calls
// it if the caller did not).
int gd_piece_inflated(vgan_gamdev *g);
int gd_piece_parse(vgan_gamdev *g, const GdCarry &in, bool last, GdCarry *out, int keep_unmapped, void (*frame_done)(void *), void *user);
// Duplicate marks of the piece's reads against the reads of the piece itself and the keys of every piece before it (`seen`, updated);
// added (or null): the keys the piece adds, for the other lanes' sets.
int gd_piece_mark_duplicates(vgan_gamdev *g, GdSeen &seen, GdKeyList *added, int64_t *n_dup);
// the keys another lane's piece added go into this lane's set
int gd_seen_merge(vgan_gamdev *g, GdSeen &seen, const GdKeyList &keys);

// ---- the pipeline over a file's pieces (gam_pipe.hip)
// What a subcommand does with a parsed piece (its arrays on the device: gamdev_slice): called on the piece's slot thread, pieces of
// different slots at the same time -- the consumer serialises what it must.  d_dup: the piece's duplicate marks (device, per read), or null.
struct GamConsumer {
    virtual ~GamConsumer() {}
    virtual int consume(int lane, vgan_gamdev *g, uint64_t read_base, const uint8_t *d_dup, int64_t piece) = 0;
    virtual void aborted() {} // the pipeline failed elsewhere: a consume that waits must give up
};
int gampipe_run(const void *bytes, uint64_t n, const std::vector<int> &lane_devices, const vgan_gampipe_opts &opts, GamConsumer &consumer,
                vgan_gampipe_stats *stats);
// the options a run takes when the caller leaves them open (piece size from the input's size, slots, tail room; VGAN_GAMPIPE_* environment)
vgan_gampipe_opts gampipe_defaults(const vgan_gampipe_opts *o, uint64_t n_bytes, int n_lanes);

inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// ---- a subcommand's run over the pipeline (vgan_<tool>_gam_start / attach / finish): the pipeline starts on a coordinator thread before
// the subcommand has its contexts; its pieces wait in consume() until attach brings them.  The reads the device flatten of a piece leaves
// go through the host on jobs of their own, joined at the finish.
struct GamJob {
    std::thread t;
    int rc = VGAN_OK;
    std::string err;
};
template <class Ctx, class Flat, class Job = GamJob> struct GamRun : GamConsumer {
    const char *tool = ""; // (the C-ABI's name: vgan_<tool>_gam_*)
    std::vector<int> devices;
    const void *bytes = nullptr;
    uint64_t n = 0;
    vgan_gampipe_opts opts{};
    std::thread coord;
    int rc = VGAN_OK;
    std::string err;
    vgan_gampipe_stats pst{};
    // what attach brings
    std::mutex mu;
    std::condition_variable cv;
    bool attached = false, gave_up = false;
    std::vector<Ctx *> ctx;
    const vgan_graph *graph = nullptr;
    std::vector<Flat *> df;         // per lane, made by its first piece
    std::deque<std::mutex> lane_mu; // (the lane's context, its stream and its flatten object: one piece at a time)
    std::vector<std::shared_ptr<Job>> bg;
    uint64_t n_host_reads = 0, n_device_reads = 0;
    double ms_wait_contexts = 0;
    int host_threads = 2;

    void aborted() override {
        {
            std::lock_guard<std::mutex> lk(mu);
            gave_up = true;
        }
        cv.notify_all();
    }
    // consume()'s prologue: waits for the contexts; the piece's read count (< 2^32 reads in the file), or an error
    int64_t piece_reads(vgan_gamdev *g, uint64_t read_base) {
        {
            const auto t0 = std::chrono::steady_clock::now();
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return attached || gave_up; });
            if (!attached) return fail(VGAN_ESTATE, "vgan_%s_gam: no contexts were attached", tool);
            ms_wait_contexts = std::max(ms_wait_contexts, ms_since(t0));
        }
        uint64_t sz[8];
        (void)vgan_gamdev_sizes(g, sz, nullptr);
        if (read_base + sz[2] > 0xFFFFFFF0ull) return fail(VGAN_ERANGE, "vgan_%s_gam: more than 2^32 reads", tool);
        return (int64_t)sz[2];
    }
    // the finish's start: nobody brings contexts any more (the pieces that wait for them give up), the pipeline and the host's jobs are
    // joined, the first error kept
    void join() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!attached) gave_up = true;
        }
        cv.notify_all();
        if (coord.joinable()) coord.join();
        for (auto &j : bg) {
            if (j->t.joinable()) j->t.join();
            if (j->rc < 0 && rc >= 0) {
                rc = j->rc;
                err = "the reads left to the host: " + j->err;
            }
        }
        pst.n_host_reads = n_host_reads;
        pst.n_device_reads = n_device_reads;
        pst.ms_wait_contexts = ms_wait_contexts;
    }
};

// vgan_<tool>_gam_start: the pipeline on its coordinator thread.  set_up: the subcommand's own options and members, before it starts.
template <class Run, class SetUp>
int gamrun_start(const char *tool, const int *devices, int n_lanes, const void *bytes, uint64_t n, const vgan_gampipe_opts *opts, Run **out, SetUp set_up) {
    if (!devices || n_lanes <= 0 || (!bytes && n) || !out) return fail(VGAN_EINVAL, "vgan_%s_gam_start: null argument", tool);
    auto *r = new Run();
    r->tool = tool;
    r->devices.assign(devices, devices + n_lanes);
    r->bytes = bytes;
    r->n = n;
    r->opts = gampipe_defaults(opts, n, n_lanes);
    r->df.assign((size_t)n_lanes, nullptr);
    r->lane_mu.resize((size_t)n_lanes);
    set_up(*r);
    const int cpus = r->opts.n_threads > 0 ? r->opts.n_threads : (int)usable_cpus();
    r->host_threads = std::max(1, std::min(8, cpus / std::max(1, n_lanes * r->opts.slots)));
    r->coord = std::thread([r] {
        r->rc = gampipe_run(r->bytes, r->n, r->devices, r->opts, *r, &r->pst);
        if (r->rc < 0) r->err = last_error();
    });
    *out = r;
    return VGAN_OK;
}

// vgan_<tool>_gam_attach: the contexts (one per lane) and the graph the waiting pieces need
template <class Ctx, class Flat, class Job>
int gamrun_attach(const char *tool, GamRun<Ctx, Flat, Job> *r, Ctx *const *ctxs, int n_ctx, const vgan_graph *graph) {
    if (!r || !ctxs || !graph) return fail(VGAN_EINVAL, "vgan_%s_gam_attach: null argument", tool);
    if (n_ctx != (int)r->devices.size()) return fail(VGAN_EINVAL, "vgan_%s_gam_attach: %d contexts for %zu lanes", tool, n_ctx, r->devices.size());
    {
        std::lock_guard<std::mutex> lk(r->mu);
        if (r->attached) return fail(VGAN_ESTATE, "vgan_%s_gam_attach: called twice", tool);
        r->ctx.assign(ctxs, ctxs + n_ctx);
        r->graph = graph;
        r->attached = true;
    }
    r->cv.notify_all();
    return VGAN_OK;
}

// The reads of a piece the device flatten leaves to the host (euka, soibean): their messages come down on the slot thread -- the piece's
// object is the next piece's once consume() returns -- and are parsed behind its back.
struct LeftReads {
    std::vector<uint32_t> where; // the reads' places among the file's mapped reads (empty: the device took every read)
    std::vector<uint64_t> offs;
    std::vector<uint8_t> msgs;
    int pick(vgan_gamdev *g, const uint8_t *mask, uint64_t R, uint64_t read_base, const char *tool);
    // one alnset of as many reads as messages (the messages are let go)
    int parse(int n_threads, const char *tool, vgan_alnset &merged);
};
} // namespace gd
} // namespace vgan
struct vgan_hc_devflat;
namespace vgan {
size_t hc_devflat_device_bytes(const vgan_hc_devflat *f); // hc_flatten_kernels.hip
}
