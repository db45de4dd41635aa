// solver.cpp -- device-resident HPR-LP solve on one GPU or one rank of a row-partitioned job.
//
// Host orchestration only: every vector operation is a kernel from kernels.hip on `stream`; the host
// synchronises exactly where the reference does (one scalar fetch per residual evaluation / sigma
// update, reference src/utils.cu:65-69).  Normal iterations between two residual evaluations are
// replayed from captured hipGraphs of 2 launches per iteration.
#include "solver.h"
#include "env.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iomanip>
#include <iostream>
#include <limits>
#include <thread>

#include "dist.h"
#include "reorder.h"

namespace hprlp {

constexpr int kMaxGraphIters = 64;
constexpr int kDeviceStartRows = 1000000;  // power iteration: start vectors longer than this are generated on the device
constexpr int kPowerBlockKey = -10;  // Solver::graphs: the power iteration's block of ten iterations (positive keys: normal iterations)

// ------------------------------------------------------------------------------------------------
// cuts (optional): for rows that are to be split at given entries -- row index -> ascending chunk starts relative to the row's
// first entry (the first one is 0) and the XCD share (0..7) each chunk should run on, -1 for "anywhere".  See slab_cuts().
struct RowCuts {
    std::vector<int> rows;                 // ascending
    std::vector<std::vector<int>> starts;  // per row
    std::vector<std::vector<int>> share;   // per chunk
    int find(int r) const {
        const auto it = std::lower_bound(rows.begin(), rows.end(), r);
        return it != rows.end() && *it == r ? static_cast<int>(it - rows.begin()) : -1;
    }
};

static std::vector<int4> build_row_blocks_cut(int rows, const int *rowptr, std::vector<int4> *longrows, const RowCuts *cuts) {
    std::vector<int4> blk;
    std::vector<int> blk_share;  // wanted XCD share of a block, -1: none
    blk.reserve(static_cast<size_t>(rows) / 8 + 16);
    // block shape: at most cap_rows rows and cap_nnz nonzeros per wave (tuning knobs; the kernel needs
    // rows <= kStreamRows and nonzeros <= kStreamW)
    // measured (tools/latency_probe.py, config 3): launch-latency-bound matrices run 9 % faster with twice
    // as many, half as long blocks (256: 15.9 us/iteration, 512: 17.4, 128: 16.0); large ones stream best at 512
    int cap_rows = kStreamRows, cap_nnz = (rows > 0 && rowptr[rows] < (1 << 22)) ? kStreamW / 2 : kStreamW;
    if (const char *e = env_get("HPRLP_STREAM_ROWS")) cap_rows = std::min(kStreamRows, std::max(1, std::atoi(e)));
    if (const char *e = env_get("HPRLP_STREAM_NNZ")) cap_nnz = std::min(kStreamW, std::max(16, std::atoi(e)));
    int r = 0, slots = 0;
    while (r < rows) {
        const int len = rowptr[r + 1] - rowptr[r];
        const int cq = (cuts && longrows) ? cuts->find(r) : -1;
        if (cq >= 0) {
            // a dense row cut where its columns cross into another XCD's eighth of the gathered vector (slab_cuts)
            const std::vector<int> &st = cuts->starts[cq];
            const int first = slots;
            for (size_t q = 0; q < st.size(); ++q) {
                const int b0 = st[q], e0 = q + 1 < st.size() ? st[q + 1] : len;
                blk.push_back(make_int4(slots++, 0, rowptr[r] + b0, e0 - b0));
                blk_share.push_back(cuts->share[cq][q]);
            }
            longrows->push_back(make_int4(r, first, slots, 0));
            ++r;
            continue;
        }
        if (len > kSplitRow && longrows) {
            // a dense row/column (LPs have them): kSplitRow-sized chunks on separate waves, descriptor
            // {chunk slot, 0, first nonzero, count}; the row itself is finished by k_long_finish
            const int first = slots;
            for (int k = rowptr[r]; k < rowptr[r + 1]; k += kSplitRow) {
                blk.push_back(make_int4(slots++, 0, k, std::min(kSplitRow, rowptr[r + 1] - k)));
                blk_share.push_back(-1);
            }
            longrows->push_back(make_int4(r, first, slots, 0));
            ++r;
            continue;
        }
        if (len > kLongRow) {
            blk.push_back(make_int4(r, 1, rowptr[r], len));
            blk_share.push_back(-1);
            ++r;
            continue;
        }
        const int start = r;
        int nz = 0;
        while (r < rows && r - start < cap_rows) {
            const int l2 = rowptr[r + 1] - rowptr[r];
            if (l2 > kLongRow || (nz + l2 > cap_nnz && r > start)) break;
            nz += l2;
            ++r;
        }
        blk.push_back(make_int4(start, r - start, rowptr[start], nz));
        blk_share.push_back(-1);
    }
    // The stream kernel gives every XCD a contiguous eighth of the block list (kernels.hip: k_spmv_fused), and a vector-mode
    // block -- a long row or a chunk of a split row -- is up to eight times the work of a stream block.  LPs carry such rows
    // in bunches (linking constraints at the end of a block-angular model: 400 chunk blocks in the last XCD's range made that
    // XCD's share 1.6 x the others').  Chunks with a wanted share go to the front of that share (their columns lie in the
    // eighth of the vector that share's rows mostly read: one L2 holds it); the other heavy blocks are spread evenly; light
    // blocks keep their order (neighbouring rows stay neighbours); split-row chunk slots keep ascending inside a share.
    const size_t N = blk.size();
    if (N >= 256) {
        std::vector<int4> light, heavy, pinned[8];
        for (size_t i = 0; i < N; ++i) {
            const int4 &d = blk[i];
            if (blk_share[i] >= 0) pinned[blk_share[i] & 7].push_back(d);
            else if (d.y == 0 || (d.y == 1 && d.w > kLongRow)) heavy.push_back(d);
            else light.push_back(d);
        }
        size_t npinned = 0;
        for (int x = 0; x < 8; ++x) npinned += pinned[x].size();
        if ((!heavy.empty() || npinned > 0) && !light.empty()) {
            // the shares' block ranges, as k_spmv_fused maps them: grid = ceil(N / 4) workgroups of 4 blocks
            const size_t grid = (N + kWavesPerBlock - 1) / kWavesPerBlock, per_lo = grid >> 3, rem = grid & 7;
            size_t ih = 0, il = 0, pos = 0;
            const size_t rest = N - npinned, H = heavy.size();
            size_t placed_rest = 0;  // light + evenly spread heavy blocks placed so far
            for (int x = 0; x < 8; ++x) {
                const size_t wg0 = x * per_lo + std::min<size_t>(x, rem), wg1 = wg0 + per_lo + (static_cast<size_t>(x) < rem ? 1 : 0);
                const size_t end = std::min(N, wg1 * kWavesPerBlock);
                size_t ip = 0;
                while (pos < end) {
                    if (ip < pinned[x].size()) {
                        blk[pos++] = pinned[x][ip++];
                        continue;
                    }
                    // heavy block ih belongs at position ih * rest / H of the unpinned sequence
                    if (ih < H && (il >= light.size() || ih * rest / H <= placed_rest)) blk[pos++] = heavy[ih++];
                    else if (il < light.size()) blk[pos++] = light[il++];
                    else break;
                    ++placed_rest;
                }
                // pinned chunks that did not fit their share (more of them than the share holds) spill into the next one
                if (ip < pinned[x].size()) {
                    std::vector<int4> &nx = pinned[std::min(x + 1, 7)];
                    if (x < 7) nx.insert(nx.begin(), pinned[x].begin() + static_cast<long>(ip), pinned[x].end());
                    else throw std::runtime_error("row blocks: pinned chunks exceed the block list");
                }
            }
            if (pos != N || ih != H || il != light.size()) throw std::runtime_error("row blocks: arrangement lost a block");
        }
    }
    return blk;
}

std::vector<int4> build_row_blocks(int rows, const int *rowptr, std::vector<int4> *longrows) {
    return build_row_blocks_cut(rows, rowptr, longrows, nullptr);
}

// Dense rows of a large matrix, cut at the columns where the gathered vector's XCD eighths meet.  A row of thousands of entries
// gathers from all over the vector: every gather pulls a 128-byte line into the L2 of whichever XCD runs the chunk, and 200
// such rows (linking constraints) were a third of the y-half's memory traffic on the block-angular ladder point.  Chunks by
// column eighth, each run by the XCD whose own rows read that eighth anyway: the lines are fetched once.  cols_of(row, out):
// the row's column indices (host copy or a download).
constexpr int kSlabSplitMin = 2048;   // rows at least this long are cut by column eighths (shorter ones: one wave, anywhere)
constexpr int kSlabChunkMin = 96;     // a chunk shorter than this joins its predecessor
template <class ColsOf>
static RowCuts slab_cuts(int rows, int cols, const int *rp, ColsOf cols_of) {
    RowCuts rc;
    const int W = (cols + 7) / 8;
    std::vector<int> ci;
    for (int r = 0; r < rows; ++r) {
        const int len = rp[r + 1] - rp[r];
        if (len < kSlabSplitMin) continue;
        ci.resize(static_cast<size_t>(len));
        cols_of(r, ci.data());
        std::vector<int> st{0}, sh{std::min(ci[0] / W, 7)};
        for (int k = 1; k < len; ++k) {
            const int slab = std::min(ci[k] / W, 7);
            const bool too_long = k - st.back() >= kSplitRow;
            if ((slab != sh.back() && k - st.back() >= kSlabChunkMin) || too_long) {
                st.push_back(k);
                sh.push_back(slab);
            }
        }
        // a short tail joins its predecessor -- unless the joined chunk would pass the split-row limit (a 4100-entry row in one
        // eighth: [0,4096) + [4096,4100) stays two chunks)
        if (st.size() > 1 && len - st.back() < kSlabChunkMin && len - st[st.size() - 2] <= kSplitRow) {
            st.pop_back();
            sh.pop_back();
        }
        rc.rows.push_back(r);
        rc.starts.push_back(std::move(st));
        rc.share.push_back(std::move(sh));
    }
    return rc;
}

// The kernels trust the block list: every chunk slot exactly once, chunk and block sizes within what a wave handles.
// Returns the number of chunk slots.
static int check_row_blocks(const std::vector<int4> &b) {
    int nslots = 0;
    std::vector<char> seen;
    for (const int4 &d : b) {
        const bool vec = d.y == 0 || (d.y == 1 && d.w > kLongRow);
        if (d.y == 0) {
            // (chunk slots: each exactly once -- the arrangement by XCD shares moves chunks, k_long_finish adds a row's slots in order)
            if (d.w < 1 || d.w > kSplitRow || d.x < 0) throw std::runtime_error("bad split-row block");
            if (static_cast<size_t>(d.x) >= seen.size()) seen.resize(static_cast<size_t>(d.x) + 1, 0);
            if (seen[d.x]++) throw std::runtime_error("bad split-row block: slot used twice");
            ++nslots;
        } else if (!vec && (d.w > kStreamW || d.y > kStreamRows || d.y < 1)) {
            throw std::runtime_error("bad row block");
        }
    }
    if (static_cast<size_t>(nslots) != seen.size()) throw std::runtime_error("bad split-row blocks: slots not contiguous");
    return nslots;
}

// Host only (no device call): the stream kernel's block list of a CSR pattern as describe_when() would build it, checked.
// out: {blocks, split rows, chunk slots, rows cut by column eighths, longest chunk, entries covered}.
void row_block_plan_host(int rows, int cols, const int *rp, const int *ci, bool with_cuts, long out[6]) {
    RowCuts cuts;
    if (with_cuts) cuts = slab_cuts(rows, cols, rp, [&](int r, int *o) { std::memcpy(o, ci + rp[r], static_cast<size_t>(rp[r + 1] - rp[r]) * sizeof(int)); });
    std::vector<int4> lr;
    const std::vector<int4> b = build_row_blocks_cut(rows, rp, &lr, cuts.rows.empty() ? nullptr : &cuts);
    const int nslots = check_row_blocks(b);
    long longest = 0, covered = 0;
    for (const int4 &d : b) {
        if (d.y == 0) longest = std::max<long>(longest, d.w);
        covered += d.w;
    }
    out[0] = static_cast<long>(b.size());
    out[1] = static_cast<long>(lr.size());
    out[2] = nslots;
    out[3] = static_cast<long>(cuts.rows.size());
    out[4] = longest;
    out[5] = covered;
}

static int workgroup_slots() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus * kTileResidentPerCu;
}

// form_select.h is host-only and cannot include tiled.h: the tile geometry its rules speak of must be the kernels'
static_assert(kFormTileRows == kTileRows && kFormTileRowsMin == kTileRowsMin && kFormTileCols == kTileCols && kFormTileColsNarrow == kTileColsNarrow &&
                  kFormMaxRow == kTileMaxRow && kFormPbRowsMax == kPbRowsMax,
              "form_select.h and tiled.h disagree on the tile geometry");

// HPRLP_TIMING=1: wall time of the set-up phases on stderr
struct PhaseTimer {
    bool on;
    clock_type::time_point t0;
    PhaseTimer() : on(env_get("HPRLP_TIMING") != nullptr), t0(time_now()) {}
    void tick(const char *what) {
        if (on) std::cerr << "[timing] " << what << ": " << time_since(t0) << " s" << std::endl;
        t0 = time_now();
    }
};

// A long copy on its own stream (driven by a helper thread) as a sequence of pieces with a short sleep after each.  While a
// pageable-memory copy is inside the HIP runtime, other threads' runtime calls wait for it: beside one 1.6 GB copy the device build
// of the tiled copy stood still for 20 ms at its first stream wait, and back-to-back pieces starved it just the same.  With the
// sleep the waiting thread gets its turn (measured on config 5, warm process: set-up of A 89 -> 67 ms; 16 / 32 / 64 MB pieces
// with 30 / 100 us equal within 3 ms).  HPRLP_COPY_PIECE_MB / HPRLP_COPY_PAUSE_US: for measurements.
static hipError_t copy_in_pieces(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t cs) {
    static const size_t kPiece = size_t(env_get("HPRLP_COPY_PIECE_MB") ? std::max(1, std::atoi(env_get("HPRLP_COPY_PIECE_MB"))) : 64) << 20;
    static const int pause_us = env_get("HPRLP_COPY_PAUSE_US") ? std::atoi(env_get("HPRLP_COPY_PAUSE_US")) : 100;
    for (size_t off = 0; off < bytes; off += kPiece) {
        const size_t len = std::min(kPiece, bytes - off);
        hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, len, kind, cs);
        if (e == hipSuccess) e = hipStreamSynchronize(cs);
        if (e != hipSuccess) return e;
        if (pause_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(pause_us));
    }
    return hipSuccess;
}

void DeviceMatrix::upload(int rows, int cols, const int *rp, const int *ci, const double *v, std::shared_ptr<void> keep) {
    PhaseTimer pt;
    const int nnz = rp[rows];
    // the kernels index without bounds checks: refuse anything that could fault on the device
    for (int i = 0; i < rows; ++i)
        if (rp[i + 1] < rp[i]) throw std::runtime_error("row pointer array is not monotone");
    const bool check_on_device = nnz > 4000000;  // (a pass over the uploaded copy: 0.3 ms instead of 10 ms of 8 host threads at 2e8)
    if (!check_on_device) {
        for (long k = 0; k < nnz; ++k)
            if (ci[k] < 0 || ci[k] >= cols) throw std::runtime_error("column index out of range");
    }
    pt.tick("  validate indices");
    rowptr.alloc(static_cast<size_t>(rows) + 1);
    rowptr.upload(rp, static_cast<size_t>(rows) + 1);
    col.alloc(nnz);
    col.upload(ci, nnz);
    if (check_on_device) {
        DBuf<int> bad;
        bad.alloc_zero(1);
        launch_check_columns(nnz, cols, col.p, bad.p, nullptr);
        int b = 0;
        bad.download(&b, 1);
        if (b) throw std::runtime_error("column index out of range");
    }
    val.alloc(nnz);
    // The values are not needed before the tiled copy is filled (or, without one, before describe() returns): a large array
    // travels on a copy stream of its own, driven by a helper thread, beside the host-side row blocks and the device build
    // of the tiled copy, which work on the index arrays (config 5: 27 ms of 1.6 GB hidden).
    std::future<void> val_job;
    if (nnz > 4000000 && env_get("HPRLP_NO_SETUP_OVERLAP") == nullptr) {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        double *dst = val.p;
        val_job = std::async(std::launch::async, [dev, dst, v, nnz]() {
            HIP_CHECK(hipSetDevice(dev));
            hipStream_t cs = nullptr;
            HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
            const hipError_t e = copy_in_pieces(dst, v, static_cast<size_t>(nnz) * sizeof(double), hipMemcpyHostToDevice, cs);
            (void)hipStreamDestroy(cs);
            HIP_CHECK(e);
        });
    } else {
        val.upload(v, nnz);
    }
    pt.tick("  upload CSR (values may still be in flight)");
    std::promise<const int *> have_rp;
    have_rp.set_value(rp);
    describe_when(rows, cols, nnz, have_rp.get_future().share(), ci, std::move(keep), -1.0, &val_job);
}

void DeviceMatrix::describe(int rows, int cols, const int *rp, const int *ci, std::shared_ptr<void> keep, double min_dense_override) {
    std::promise<const int *> have_rp;
    have_rp.set_value(rp);
    describe_when(rows, cols, rp[rows], have_rp.get_future().share(), ci, std::move(keep), min_dense_override, nullptr);
}

// Row blocks, kernel views and the tiled copy, for a matrix whose CSR arrays are already in rowptr / col / val on the device.
// rp_ready delivers the same row pointers on the host (for A^T after a device transpose: when their download, running in a thread
// of the caller, is done); ci: the host column indices or null.  The row blocks of the stream kernel are a host-side walk over the
// row pointers (13-18 ms at 1e7 rows): a job of their own beside the device build of the tiled copy, which reads only the device
// arrays.  values_ready (optional): the upload of val still in flight -- joined before the first use of the values.
void DeviceMatrix::describe_when(int rows, int cols, long nnz_l, std::shared_future<const int *> rp_ready, const int *ci, std::shared_ptr<void> keep,
                                 double min_dense_override, std::future<void> *values_ready) {
    PhaseTimer pt;
    view.longrows = nullptr;  // (describe() may run again on a permuted copy of the matrix: start from a clean view)
    view.nlong = 0;
    view.long_partial = nullptr;
    view.tiled = TiledDev();
    const int nnz = static_cast<int>(nnz_l);
    auto host_rp = [&rp_ready]() { return rp_ready.get(); };
    auto join_values = [values_ready]() {
        if (values_ready && values_ready->valid()) values_ready->get();
    };
    struct Blocks {
        std::vector<int4> b, lr;
    };
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const int *dcol = col.p;
    // dense rows of a matrix whose gathered vector is beyond one L2: cut by column eighths (slab_cuts); the column indices of
    // those rows come from the host copy or, for a matrix built on the device, from a download of just those rows
    auto make_blocks = [rows, cols, nnz, rp_ready, ci, dev, dcol]() {
        HIP_CHECK(hipSetDevice(dev));
        const int *rp = rp_ready.get();
        RowCuts cuts;
        const char *noslab = env_get("HPRLP_NO_SLAB_CUTS");
        if (cols >= (1 << 19) && nnz >= (1 << 22) && !(noslab && noslab[0] == '1')) {
            cuts = slab_cuts(rows, cols, rp, [&](int r, int *out) {
                const size_t len = static_cast<size_t>(rp[r + 1] - rp[r]);
                if (ci) std::memcpy(out, ci + rp[r], len * sizeof(int));
                else HIP_CHECK(hipMemcpy(out, dcol + rp[r], len * sizeof(int), hipMemcpyDeviceToHost));
            });
        }
        Blocks out;
        out.b = build_row_blocks_cut(rows, rp, &out.lr, cuts.rows.empty() ? nullptr : &cuts);
        return out;
    };
    const bool overlap = rows > 100000 && env_get("HPRLP_NO_SETUP_OVERLAP") == nullptr;
    std::future<Blocks> blocks_job = std::async(overlap ? std::launch::async : std::launch::deferred, make_blocks);
    view.rows = rows;
    view.cols = cols;
    view.nnz = nnz;
    view.rowptr = rowptr.p;
    view.col = col.p;
    view.val = val.p;
    // nontemporal matrix loads only when the matrix cannot stay in the eight 4 MiB L2s anyway
    view.nt = static_cast<size_t>(nnz) * 12 > (static_cast<size_t>(16) << 20);
    if (const char *e = env_get("HPRLP_NT")) view.nt = std::atoi(e) != 0;
    try {
        longest_row = 0;
        double long_row_share = 0.0;  // share of the entries in rows of more than kSkewRow entries (0 for small matrices)
        if (rows > 100000) {  // (from the device copy: the host row pointers of A^T may still be on their way)
            long in_long = 0;
            longest_row = launch_longest_row(rowptr.p, rows, nullptr, kSkewRow, &in_long);
            long_row_share = nnz > 0 ? static_cast<double>(in_long) / nnz : 0.0;
        } else {
            const int *rp = host_rp();
            for (int i = 0; i < rows; ++i) longest_row = std::max(longest_row, rp[i + 1] - rp[i]);
        }
        build_tiled_copy(rows, cols, nnz, long_row_share, host_rp, ci, std::move(keep), min_dense_override, join_values, pt);
        join_values();
    } catch (...) {
        if (blocks_job.valid()) blocks_job.wait();
        throw;
    }
    Blocks B = blocks_job.get();
    std::vector<int4> &b = B.b, &lr = B.lr;
    const int nslots = check_row_blocks(b);
    blk.alloc(b.size());
    blk.upload(b.data(), b.size());
    pt.tick("  row blocks");
    if (!lr.empty()) {
        longrows.alloc(lr.size());
        longrows.upload(lr.data(), lr.size());
        long_partial.alloc_zero(static_cast<size_t>(nslots) * 2);
        view.longrows = longrows.p;
        view.nlong = static_cast<int>(lr.size());
        view.long_partial = long_partial.p;
    }
    view.blk = blk.p;
    view.nblk = static_cast<int>(b.size());
}

static FormBuilt built_figures(const DeviceTiled &t, bool ok) {
    FormBuilt b = {ok ? 1L : 0L, t.view.n_pieces, static_cast<long>(t.dense_entries), static_cast<long>(t.n_rem), t.rem_top_share};
    return b;
}

// The tiled copy of describe_when(): measure, ask the rules (form_select.h), build on the device (or start the host builder's
// background job), ask again, keep the copy and fill in its values -- or drop it.
void DeviceMatrix::build_tiled_copy(int rows, int cols, int nnz, double long_row_share, const std::function<const int *()> &host_rp, const int *ci,
                                    std::shared_ptr<void> keep, double min_dense_override, const std::function<void()> &join_values, PhaseTimer &pt) {
    const FormHooks hk = read_form_hooks();
    if (hk.no_tiled) return;  // (outcome and facts stay as they are)
    // (a stream of its own for the build was measured: the stall beside the value upload is the runtime's lock, not a stream wait)
    const hipStream_t bs = nullptr;
    const int rb = sb_rows, gb = far_group;  // (heights, not bit counts)
    passes = min_dense_override >= 0.0 ? 2 : 1;
    FormFacts &f = passes == 2 ? facts_pb : facts;
    f = blank_form_facts();
    f.rows = rows;
    f.cols = cols;
    f.nnz = nnz;
    f.longest_row = longest_row;  // (describe_when)
    f.long_row_share = long_row_share;
    f.xcd_gather_bytes = xcd_gather_bytes;
    f.sb_rows = rb;
    f.slots = workgroup_slots();
    f.min_dense_override = min_dense_override;
    if (rows >= 8192 && nnz > 1000000) f.line_density = launch_line_density(rowptr.p, col.p, rows, nullptr);
    if (pt.on) std::cerr << "[timing]   gathered 64-byte lines per entry (sampled 64-row windows): " << f.line_density << std::endl;
    PreBuild p;
    for (;;) {  // a pass that an earlier rule makes unnecessary does not run
        p = before_build(f, hk);
        if (p.need == FormNeed::HeaviestBlock) f.heaviest_block = launch_heaviest_block(rowptr.p, rows, rb, nullptr);
        else if (p.need == FormNeed::TilingShare) f.tiling_share = device_tiling_dense_fraction(rows, cols, nnz, rowptr.p, col.p, nullptr, nullptr, bs);
        else break;
    }
    if (pt.on && (p.skew || p.imbalance))
        std::cerr << "[timing]   tiled forms declined for the row lengths: " << (p.skew ? "skew" : "imbalance") << " (share of the entries in rows over "
                  << kSkewRow << ": " << long_row_share << ")" << std::endl;
    if (pt.on && f.tiling_share >= 0.0)
        std::cerr << "[timing]   thin rows (" << p.entries_per_row << " per row), tiling test: " << f.tiling_share << " of the entries in dense tiles" << std::endl;
    if (p.thin_early) {
        route_of(f, p, &outcome);
        pt.tick("  tiling test (thin rows: the stream kernel without a build)");
        return;
    }
    auto adopt = [&]() {
        view.tiled = tiled.view;
        join_values();
        launch_tiled_refresh(tiled, val.p, bs);
        HIP_CHECK(hipDeviceSynchronize());
    };
    if (p.side_open) {
        const int *rp = host_rp();
        std::vector<int> long_rows;
        long long_nnz = 0;
        for (int i = 0; i < rows; ++i)
            if (rp[i + 1] - rp[i] > kTileMaxRow) {
                long_rows.push_back(i);
                long_nnz += rp[i + 1] - rp[i];
            }
        f.n_long_rows = static_cast<long>(long_rows.size());
        f.long_rows_nnz = long_nnz;
        if (long_rows_aside(f)) {
            std::vector<int> rp_c(static_cast<size_t>(rows) + 1, 0);
            for (int i = 0; i < rows; ++i) {
                const int len = rp[i + 1] - rp[i];
                rp_c[i + 1] = rp_c[i] + (len > kTileMaxRow ? 0 : len);
            }
            const long nnz_c = rp_c[rows];
            DBuf<int> d_rp_c(rp_c.size()), col_c(static_cast<size_t>(std::max<long>(nnz_c, 1))), map_c(static_cast<size_t>(std::max<long>(nnz_c, 1)));
            d_rp_c.upload(rp_c.data(), rp_c.size());
            compact_without_rows(nnz, rows, rowptr.p, d_rp_c.p, col.p, col_c.p, map_c.p, bs);
            const bool ok = tiled.build_on_device(rows, cols, nnz_c, d_rp_c.p, col_c.p, p.min_rows, p.min_dense, bs, rb, tile_cols, rem_cap);
            f.side = built_figures(tiled, ok);
            if (pt.on)
                std::cerr << "[timing]   tiled copy without " << long_rows.size() << " long rows (" << long_nnz << " entries, longest " << longest_row
                          << "): " << (ok ? "" : "declined; ") << tiled.view.nsb << " super-blocks, " << tiled.n_steps << " steps" << std::endl;
            const bool kept = after_build(f, hk, p, f.side, true, false) == NoTiled::None;
            if (ok && !kept) tiled = DeviceTiled();
            if (kept) {
                tiled.build_far(cols, bs, gb);
                tiled.compose_perms(map_c.p, bs);
                tiled.set_side(rows, rp, long_rows);
                adopt();
                outcome = FormOutcome();
            }
            pt.tick("  build tiled copy (device, long rows aside)");
            if (kept) return;
        }
    }
    switch (route_of(f, p, &outcome)) {
        case FormRoute::NotAttempted:
            if (pt.on) std::cerr << "[timing]   tiled copy not attempted: " << cols << " columns, longest row " << longest_row << std::endl;
            break;
        case FormRoute::FewRows:
            if (pt.on) std::cerr << "[timing]   tiled copy not attempted: " << rows << " rows (staged tiles from " << p.min_rows << " on)" << std::endl;
            break;
        case FormRoute::DeviceBuild: {
            // built on the device from the device CSR arrays (tiled_build.hip); HPRLP_TILING_CHECK=1 also runs the
            // host builder and compares every array
            const bool ok = tiled.build_on_device(rows, cols, nnz, rowptr.p, col.p, p.min_rows, p.min_dense, bs, rb, tile_cols, rem_cap);
            f.whole = built_figures(tiled, ok);
            if (pt.on)
                std::cerr << "[timing]   tiled copy (device build): " << (ok ? "" : "declined; ") << tiled.view.nsb << " super-blocks, "
                          << tiled.n_steps << " steps, " << tiled.dense_entries << " entries in tiles + " << tiled.padding
                          << " padding, " << tiled.n_rem << " in the remainder list" << std::endl;
            if (hk.tiling_check == 1 && ci) {
                TiledHost th;
                const bool hok = build_tiled(rows, cols, host_rp(), ci, &th, p.min_rows, p.min_dense, rb, tile_cols, rem_cap);
                if (hok != ok) throw std::runtime_error("tiling check: host and device builders disagree on acceptance");
                if (ok) tiled.compare_with(th);
            }
            NoTiled why = after_build(f, hk, p, f.whole, false, false);
            if (why == NoTiled::None) {
                tiled.build_far(cols, bs, gb);  // consumes the remainder lists the check above compares
                f.whole.rem_top_share = tiled.rem_top_share;
                why = after_build(f, hk, p, f.whole, false, true);
            }
            if (ok && why != NoTiled::None) {
                if (pt.on && why == NoTiled::Sparse) std::cerr << "[timing]   piece form with " << staged_share(f.whole) << " of the entries in staged tiles: declined" << std::endl;
                if (pt.on && why == NoTiled::Thin) std::cerr << "[timing]   piece form with " << p.entries_per_row << " entries per row: the stream kernel instead" << std::endl;
                if (pt.on && why == NoTiled::Popular)
                    std::cerr << "[timing]   " << tiled.rem_top_share << " of the remainder on 2 MB of popular columns, window in one L2: the stream kernel instead" << std::endl;
                tiled = DeviceTiled();
            }
            outcome.why = why;
            if (why == NoTiled::None) adopt();
            pt.tick("  build tiled copy (device)");
            break;
        }
        case FormRoute::HostBuild:
            if (ci) {  // the host builder needs the host column indices
                planned_grid = std::max(((rows + rb - 1) / rb + 7) / 8 * 8, (rows + kThreads - 1) / kThreads);  // fused grid or the split form's finish grid
                const int tc = tile_cols, rc = rem_cap, min_rows = p.min_rows;
                const double min_dense = p.min_dense;
                const int *rp = host_rp();
                tiling = std::async(std::launch::async, [=]() -> std::shared_ptr<TiledHost> {
                    (void)keep;  // keeps the host arrays alive for the duration of the build
                    auto th = std::make_shared<TiledHost>();
                    return build_tiled(rows, cols, rp, ci, th.get(), min_rows, min_dense, rb, tc, rc) ? th : nullptr;
                });
            }
            break;
        default:
            break;
    }
}

void DeviceMatrix::finish_tiling(hipStream_t s) {
    if (!tiling.valid()) return;
    PhaseTimer pt;
    std::shared_ptr<TiledHost> th = tiling.get();  // rethrows what the job threw
    pt.tick("  wait for the tiled build");
    if (!th) {
        planned_grid = 0;
        return;
    }
    if (pt.on)
        std::cerr << "[timing]   tiled copy: " << th->sb_mid.size() << " super-blocks, " << th->steps.size() << " steps, "
                  << th->dense_entries << " entries in tiles + " << th->padding << " padding, " << th->n_rem
                  << " in the remainder list" << std::endl;
    tiled.upload(*th, sb_rows, tile_cols, rem_cap);
    tiled.build_far(view.cols, s, far_group);
    view.tiled = tiled.view;
    launch_tiled_refresh(tiled, val.p, s);
    HIP_CHECK(hipStreamSynchronize(s));
    pt.tick("  upload tiled copy");
}

void DeviceMatrix::refresh_tiled(hipStream_t s) {
    if (view.tiled.valid) launch_tiled_refresh(tiled, val.p, s);
}

// ------------------------------------------------------------------------------------------------
Solver::~Solver() {
    A.tiled.dump_stamps();
    AT.tiled.dump_stamps();
    A.tiled.dump_wgtimes();
    AT.tiled.dump_wgtimes();
    for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
    if (ev_ready) (void)hipEventDestroy(ev_ready);
    if (ev_done_x) (void)hipEventDestroy(ev_done_x);
    if (ev_done_y) (void)hipEventDestroy(ev_done_y);
    if (inputs_ready) (void)hipEventDestroy(inputs_ready);
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    if (stream && !arena) (void)hipStreamDestroy(stream);
    // (the buffers taken from the arena are not given back one by one: DBuf::release leaves them alone; the last member frees the blocks)
    if (arena) arena_release(arena);
}

bool Solver::group_setup_fits(const LP_info_cpu *model) {
    if (!model || !model->A || model->m <= 0 || model->n <= 0) return false;
    const long nnz = model->A->numElements;
    if (!small_path_fits(model->m, model->n, nnz, 0, 0)) return false;
    const char *hostt = env_get("HPRLP_HOST_TRANSPOSE");
    const char *dmin = env_get("HPRLP_DEVICE_TRANSPOSE_MIN");
    if (nnz > (dmin ? std::atol(dmin) : 4000000L) && !(hostt && hostt[0] == '1')) return false;  // (setup(): the device transpose)
    const FormHooks hk = read_form_hooks();
    // (form_select.cpp: before_build -- so few columns are "not attempted" unless a hook lowers the thresholds)
    return hk.no_tiled || (!hk.tiled_min_rows.set && !hk.tiled_min_cols.set && !hk.tiled_anyway);
}

void Solver::alloc_work() {
    x.alloc_zero(n_loc); last_x.alloc_zero(n_loc); z_bar.alloc_zero(n_loc);
    last_y.alloc_zero(m_loc); y_obj.alloc_zero(m_loc); y_temp.alloc_zero(m_loc);
    gy.alloc_zero(m_pad); gyb.alloc_zero(m_pad); gsm.alloc_zero(m_pad);
    gxh.alloc_zero(n_pad); gxb.alloc_zero(n_pad); gxt.alloc_zero(n_pad); gsn.alloc_zero(n_pad);
    y = gy.p + row_off; y_bar = gyb.p + row_off;
    x_hat = gxh.p + col_off; x_bar = gxb.p + col_off; x_temp = gxt.p + col_off;
    sm1.alloc_zero(m_loc); sn1.alloc_zero(n_loc);
    row_norm.alloc(m_loc); col_norm.alloc(n_loc);
    ctrl.alloc_zero(1);
    scal.alloc_zero(kNumScalars);
    scal_h.alloc(kNumScalars);
    stride_x = std::max(std::max(AT.view.grid(), AT.planned_grid), 1);  // either kernel's partials fit
    stride_y = std::max(std::max(A.view.grid(), A.planned_grid), 1);
    part_x.alloc_zero(static_cast<size_t>(3) * stride_x);
    part_y.alloc_zero(static_cast<size_t>(2) * stride_y);
    part_r.alloc_zero(static_cast<size_t>(2) * std::max(stride_x, stride_y));
    part_v.alloc_zero(static_cast<size_t>(2) * kReduceBlocks);
    if (arena && !hook_no_bound_codes) {  // (refresh_bound_codes would allocate them after the scope: two hipMallocs and two hipFrees per member)
        if (n_loc > 0) lu_code.alloc(static_cast<size_t>(n_loc));
        if (m_loc > 0) row_code.alloc(static_cast<size_t>(m_loc));
    }
    const char *ng = env_get("HPRLP_NO_GRAPH");
    use_graph = !(ng && ng[0] == '1') && comm == nullptr;
    const char *no = env_get("HPRLP_NO_OVERLAP");
    overlap_enabled = comm != nullptr && comm->size > 1 && !(no && no[0] == '1');
    // HPRLP_OVERLAP_COMM_FIRST=1 (tests): take RCCL's launch order with the in-process group too
    overlap_spmv_first = comm != nullptr && comm->host_blocking() && !env_get("HPRLP_OVERLAP_COMM_FIRST");
}

void Solver::setup(const LP_info_cpu *model, const HPRLP_parameters *param) {
    const auto t0 = time_now();
    prm = *param;
    env_at_setup = env_in_effect(&env_ignored_at_setup);
    read_hooks();
    HIP_CHECK(hipSetDevice(prm.device_number));
    if (Arena *a = arena_in_scope()) {
        arena = a;
        arena_retain(a);
        stream = arena_stream(a);
    } else {
        HIP_CHECK(hipStreamCreate(&stream));
    }
    m = m_loc = model->m;
    n = n_loc = model->n;
    m_pad = m; n_pad = n;
    row_off = col_off = 0;
    obj_constant = model->obj_constant;
    const sparseMatrix *As = model->A;
    if (!As || As->row != m || As->col != n) throw std::runtime_error("model matrix dimensions inconsistent");
    const long nnz = As->numElements;
    PhaseTimer pt;
    // choose_sb_rows() reads rowPtr / colIndex on the host before upload() has validated them: refuse a malformed row
    // pointer array here (upload() repeats the monotonicity test and checks the column range)
    if (!As->rowPtr || !As->colIndex || !As->value) throw std::runtime_error("model matrix arrays missing");
    if (As->rowPtr[0] != 0 || As->rowPtr[m] != nnz) throw std::runtime_error("row pointer array does not span the nonzeros");
    for (int i = 0; i < m; ++i)
        if (As->rowPtr[i + 1] < As->rowPtr[i]) throw std::runtime_error("row pointer array is not monotone");
    choose_sb_rows(model);
    A.upload(m, n, As->rowPtr, As->colIndex, As->value);
    pt.tick("A upload total");
    // the five model vectors (in the solver's numbering): uploaded beside the device build of A^T's tiled copy when the matrix is
    // large (own copy stream, helper thread), otherwise in line
    std::future<void> vec_job;
    auto upload_vectors = [this, model](bool own_stream) {
        int dev = prm.device_number;
        HIP_CHECK(hipSetDevice(dev));
        hipStream_t cs = nullptr;
        if (own_stream) HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        auto upload_vec = [cs, own_stream](DBuf<double> &d, const double *src, int len, const std::vector<int> &perm) {
            std::vector<double> tmp;
            if (!perm.empty()) {
                tmp.resize(static_cast<size_t>(len));
                for (int i = 0; i < len; ++i) tmp[i] = src[perm[i]];
                src = tmp.data();
            }
            if (own_stream) HIP_CHECK(copy_in_pieces(d.p, src, static_cast<size_t>(len) * sizeof(double), hipMemcpyHostToDevice, cs));
            else d.upload(src, len);
        };
        try {
            upload_vec(AL, model->AL, m, perm_r);
            upload_vec(AU, model->AU, m, perm_r);
            upload_vec(l, model->l, n, perm_c);
            upload_vec(u, model->u, n, perm_c);
            upload_vec(c, model->c, n, perm_c);
        } catch (...) {
            if (cs) (void)hipStreamDestroy(cs);
            throw;
        }
        if (cs) (void)hipStreamDestroy(cs);
    };
    AL.alloc(m);
    AU.alloc(m);
    l.alloc(n);
    u.alloc(n);
    c.alloc(n);
    {   // explicit A^T built on the host, stable in row order (reference src/preprocess.cu:78-82); its index
        // arrays are handed to the background job that builds the tiled copy of A^T
        struct HostT {
            std::vector<int> trp, tci;
        };
        auto ht = std::make_shared<HostT>();
        std::vector<int> &trp = ht->trp, &tci = ht->tci;
        const char *hostt = env_get("HPRLP_HOST_TRANSPOSE");
        const char *dmin = env_get("HPRLP_DEVICE_TRANSPOSE_MIN");  // nonzero threshold (tests lower it)
        if (nnz > (dmin ? std::atol(dmin) : 4000000L) && !(hostt && hostt[0] == '1')) {
            // large matrix: transpose on the device (transpose.hip), bring the index arrays back for the host-side
            // consumers (tiled build, row statistics)
            AT.rowptr.alloc(static_cast<size_t>(n) + 1);
            AT.col.alloc(static_cast<size_t>(nnz));
            AT.val.alloc(static_cast<size_t>(nnz));
            device_transposed = true;
            device_transpose(m, n, nnz, A.rowptr.p, A.col.p, A.val.p, AT.rowptr.p, AT.col.p, AT.val.p, stream);
            pt.tick("device transpose");
            const bool reordered = try_reorder(model);
            if (reordered) {  // A now holds P A Q: transpose that
                device_transpose(m, n, nnz, A.rowptr.p, A.col.p, A.val.p, AT.rowptr.p, AT.col.p, AT.val.p, stream);
                pt.tick("locality ordering + device transpose of the permuted matrix");
            }
            // (also behind an ordering whose copy the build then declined -- the cheap tiling test had accepted it: covering pattern
            // 300k x 3M, four per column: stream kernel 0.188 ms on the y-half where the remainder path takes 0.133; end of round 5)
            if (!A.view.tiled.valid && pb_fallback_wanted(A, AT.rowptr.p, n)) {
                choose_pb_rows(A, AT, m, n);
                // no column locality to be had (or the ordering is disabled): every random 8-byte gather of the stream kernel
                // would cost a 128-byte line from the Infinity Cache / HBM.  Accept the tiled form with NO dense-tile
                // requirement: whatever is not in dense tiles -- here almost everything -- goes through the propagation-
                // blocking remainder (pre-pass in source order, streamed products in destination order): about 30 bytes per
                // nonzero, all sequential.  Unstructured 2e8-nnz matrix: 3.85 -> 1.87 ms per half-step.
                if (reordered) {
                    std::vector<int> hrp(static_cast<size_t>(m) + 1);
                    A.rowptr.download(hrp.data(), hrp.size());
                    A.describe(m, n, hrp.data(), nullptr, nullptr, 0.0);
                } else {
                    A.describe(m, n, As->rowPtr, nullptr, nullptr, 0.0);
                }
                pt.tick("tiled copy of A without a dense-tile requirement (propagation blocking for all entries)");
            }
            // the host copy of A^T's row pointers (row blocks, statistics) comes back on a copy stream of its own, driven by a
            // thread, while the tiled copy of A^T is built from the device arrays (describe_when)
            int dev = 0;
            HIP_CHECK(hipGetDevice(&dev));
            const bool overlap_setup = env_get("HPRLP_NO_SETUP_OVERLAP") == nullptr;
            const int *d_trp = AT.rowptr.p;
            const int n_rows_t = n;
            std::shared_future<const int *> trp_ready =
                std::async(overlap_setup ? std::launch::async : std::launch::deferred, [ht, dev, d_trp, n_rows_t]() -> const int * {
                    HIP_CHECK(hipSetDevice(dev));
                    ht->trp.resize(static_cast<size_t>(n_rows_t) + 1);
                    hipStream_t cs = nullptr;
                    HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
                    const hipError_t e = copy_in_pieces(ht->trp.data(), d_trp, ht->trp.size() * sizeof(int), hipMemcpyDeviceToHost, cs);
                    (void)hipStreamDestroy(cs);
                    HIP_CHECK(e);
                    return ht->trp.data();
                }).share();
            // the column indices of A^T are only needed on the host by the host tiled builder (or its check)
            const FormHooks hk = read_form_hooks();
            const bool need_tci = hk.host_tiling || hk.tiling_check == 1;
            if (need_tci) {
                tci.resize(static_cast<size_t>(nnz));
                AT.col.download(tci.data(), tci.size());
            }
            if (overlap_setup) vec_job = std::async(std::launch::async, upload_vectors, true);  // (the numbering is final here)
            AT.describe_when(n, m, nnz, trp_ready, need_tci ? tci.data() : nullptr, ht, -1.0, nullptr);
            trp_ready.wait();
            if (pb_fallback_wanted(AT, A.rowptr.p, m)) {
                choose_pb_rows(AT, A, n, m);
                AT.describe(n, m, trp.data(), nullptr, nullptr, 0.0);
            }
        } else {
            std::vector<double> tv;
            csr_transpose_host(m, n, nnz, As->rowPtr, As->colIndex, As->value, trp, tci, tv);
            pt.tick("host transpose");
            AT.upload(n, m, trp.data(), tci.data(), tv.data(), ht);
        }
        pt.tick("A^T upload total");
        max_row_A = std::max(max_row_A, A.longest_row);  // (describe_when; a renumbering does not change the longest row)
        max_row_AT = std::max(max_row_AT, AT.longest_row);
        const char *ns = env_get("HPRLP_NO_SMALL");
        use_small = !(ns && ns[0] == '1') && small_path_fits(m, n, nnz, max_row_A, max_row_AT);
        if (use_small) {
            auto by_length = [](int rows, const int *rp, DBuf<int> &out) {
                std::vector<int> ord(rows);
                for (int i = 0; i < rows; ++i) ord[i] = i;
                std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return rp[a + 1] - rp[a] > rp[b + 1] - rp[b]; });
                out.alloc(rows);
                out.upload(ord.data(), rows);
            };
            by_length(n, trp.data(), small_order_x);
            by_length(m, As->rowPtr, small_order_y);
            // the transpose is stable in row order: the k-th entry of A (row i, column j) is the next free
            // slot of row j of A^T
            std::vector<int> next(trp.begin(), trp.end() - 1), ij(static_cast<size_t>(nnz)), posA(static_cast<size_t>(nnz));
            for (int i = 0; i < m; ++i)
                for (int k = As->rowPtr[i]; k < As->rowPtr[i + 1]; ++k) {
                    const int j = As->colIndex[k], q = next[j]++;
                    if (tci[q] != i) throw std::runtime_error("small path: transpose is not stable");
                    ij[q] = i | (j << 16);
                    posA[q] = k;
                }
            small_ij.alloc(ij.size());
            small_ij.upload(ij.data(), ij.size());
            small_posA.alloc(posA.size());
            small_posA.upload(posA.data(), posA.size());
        }
    }
    if (vec_job.valid()) vec_job.get();
    else upload_vectors(false);
    alloc_work();
    // the tiled copy of A was built from the model's own arrays, which the caller may free once we return; the
    // job of A^T owns its arrays and keeps running under scale()
    A.finish_tiling(stream);
    pt.tick("vectors, work space, tiled copy of A");
    if (!arena) HIP_CHECK(hipDeviceSynchronize());  // (a group waits once, after the arena's flush)
    setup_time = time_since(t0);
    if (pt.on) {
        const AllocStats &as = AllocStats::get();
        std::cerr << "[timing] allocator so far (process): " << as.mallocs << " hipMalloc " << as.malloc_s << " s, " << as.frees << " hipFree "
                  << as.free_s << " s" << std::endl;
    }
}

// Share of a matrix' entries whose gathers go to the `lines` most popular 64-byte lines of the gathered vector (columns 8 l .. 8 l + 7;
// `other` is the transpose: its row lengths are the column counts).  What the stream kernel's gathers find in an L2 however far apart
// the rows reach.
static double popular_lines_share(const int *d_rowptr, int cols, long nnz, long lines) {
    if (cols <= 0 || nnz <= 0 || !d_rowptr) return 0.0;
    std::vector<int> rp(static_cast<size_t>(cols) + 1);
    HIP_CHECK(hipMemcpy(rp.data(), d_rowptr, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
    const long nl = (static_cast<long>(cols) + 7) / 8;
    if (nl <= lines) return 1.0;
    std::vector<int> deg(static_cast<size_t>(nl));
    for (long l = 0; l < nl; ++l) deg[l] = rp[std::min<long>(8 * (l + 1), cols)] - rp[8 * l];
    std::nth_element(deg.begin(), deg.begin() + lines, deg.end(), std::greater<int>());
    long top = 0;
    for (long l = 0; l < lines; ++l) top += deg[l];
    return static_cast<double>(top) / static_cast<double>(nnz);
}

// The all-remainder decision (form_select.h: all_remainder_wanted, rules 7 and 13) on what M's last describe() left behind; the
// popular-lines download and the heaviest-block pass run only when the rule gets as far as asking for them.
bool Solver::pb_fallback_wanted(DeviceMatrix &M, const int *other_rowptr, int other_rows) {
    const FormHooks hk = read_form_hooks();
    FormFacts &f = M.facts;
    f.sharded = comm != nullptr;
    AllRemainder r;
    for (;;) {
        r = all_remainder_wanted(f, hk, M.outcome, M.view.tiled.valid);
        if (r.need == FormNeed::PopularShare) f.popular_share = popular_lines_share(other_rowptr, other_rows, M.view.nnz, kPopularLines);
        else if (r.need == FormNeed::HeaviestPbBlock) f.heaviest_pb_block = launch_heaviest_block(M.rowptr.p, M.view.rows, kPbRowsMax, stream);
        else break;
    }
    if (env_get("HPRLP_TIMING")) {
        if (f.heaviest_pb_block >= 0)
            std::cerr << "[timing] long rows: share of the entries on the " << kPopularLines << " most popular lines " << f.popular_share << ", heaviest block of " << kPbRowsMax
                      << " rows " << f.heaviest_pb_block << " entries of " << M.view.nnz << std::endl;
        else if (f.popular_share >= 0.0)
            std::cerr << "[timing] few rows: share of the entries on the " << kPopularLines << " most popular lines " << f.popular_share << std::endl;
    }
    return r.wanted;
}

// Heights for a matrix that runs the all-remainder form (form_select.h: pb_height).  Writes into BOTH matrices: a source group
// of one matrix' remainder lists is a super-block of the other.
void Solver::choose_pb_rows(DeviceMatrix &M, DeviceMatrix &other, int rows, int other_rows) {
    M.rem_cap = kTileRemCap;
    if (comm) return;
    const FormHooks hk = read_form_hooks();
    if (!hk.tile_rows.set) {
        const int slots = workgroup_slots();
        M.sb_rows = other.far_group = pb_height(rows, slots);
        // the other matrix has the same graph: if it is not described yet, expect it to take the same form (its source groups are
        // this matrix' hand-off unit, kernels.h FarPush; a wrong guess only costs the hand-off)
        if (!other.view.tiled.valid) other.sb_rows = M.far_group = pb_height(other_rows, slots);
    }
    if (pb_kernel_fits(M.sb_rows, hk)) M.rem_cap = kPbRemCap;
    if (env_get("HPRLP_TIMING"))
        std::cerr << "[timing] no column locality: all-remainder form with super-blocks of " << M.sb_rows << " rows, remainder steps of " << M.rem_cap
                  << " entries" << std::endl;
}

// Super-block heights, tile widths and the XCD window estimate of this LP's tiled copies (form_select.h: tile_shapes) from the
// median column span of a row, sampled here where the host arrays are.
void Solver::choose_sb_rows(const LP_info_cpu *model) {
    const FormHooks hk = read_form_hooks();
    const sparseMatrix *As = model->A;
    const long nnz = As->numElements;
    double w_a = 0.0;
    if (row_spans_wanted(nnz, comm != nullptr, hk)) {
        // median column span of a row without its outermost entries
        std::vector<long> span;
        const int samples = 2048;
        for (int q = 0; q < samples; ++q) {
            const int i = static_cast<int>(static_cast<long>(q) * m / samples);
            const int b = As->rowPtr[i], e = As->rowPtr[i + 1], len = e - b;
            if (len < 4) continue;
            // an eighth of the entries off either end (at least one: a 16-entry row of config 5's kind carries one far entry),
            // the span of the rest scaled back to the whole row
            // (rows need not be sorted by column: the span is |difference|, an unsorted row only makes the estimate coarser,
            // never negative -- a negative span used to pass the `ratio <= most` test below)
            const int cut = std::max(1, len / 8);
            const long ia = std::min<long>(std::max<long>(static_cast<long>(e) - 1 - cut, b), nnz - 1), ib = std::min<long>(static_cast<long>(b) + cut, nnz - 1);
            const long inner = std::labs(static_cast<long>(As->colIndex[ia]) - As->colIndex[ib]);
            span.push_back(inner * (len - 1) / std::max(1, len - 1 - 2 * cut));
        }
        if (span.size() >= 16) {
            std::nth_element(span.begin(), span.begin() + span.size() / 2, span.end());
            w_a = static_cast<double>(std::max<long>(span[span.size() / 2], 1));
        }
    }
    const int slots = w_a > 0.0 ? workgroup_slots() : 0;
    const TileShapes t = tile_shapes(m, n, nnz, slots, w_a, hk);
    A.sb_rows = AT.far_group = t.sb_rows_a;
    AT.sb_rows = A.far_group = t.sb_rows_at;
    A.tile_cols = t.tile_cols_a;
    AT.tile_cols = t.tile_cols_at;
    A.xcd_gather_bytes = t.xcd_bytes_a;
    AT.xcd_gather_bytes = t.xcd_bytes_at;
    if (env_get("HPRLP_TIMING")) {
        if (t.estimated && !hk.tile_cols.set)
            std::cerr << "[timing] entries of a row per 2048-column tile: " << t.per_tile_a << " (A), " << t.per_tile_at << " (A^T) -> tiles of "
                      << A.tile_cols << " / " << AT.tile_cols << " columns" << std::endl;
        if (t.weighed)
            std::cerr << "[timing] super-block heights for whole rounds of " << slots << " slots: " << t.ra << " (A), " << t.rat << " (A^T); median row span " << w_a
                      << " columns, tile bytes / entry bytes " << t.ratio_a << ", " << t.ratio_at << " -> " << (t.lowered ? "lowered" : "full height (8192)") << std::endl;
    }
}

// Large matrix whose given order failed the tiling test: look for a locality ordering (reorder.cpp).  On entry A (device
// CSR of the model) and the arrays of AT (device transpose, not yet described) are in place.  On success A's device
// arrays hold P A Q, A is re-described (row blocks, tiled copy) and perm_r / perm_c are set.
bool Solver::try_reorder(const LP_info_cpu *model) {
    if (!allow_reorder) return false;
    const char *no = env_get("HPRLP_NO_REORDER");
    if (no && no[0] == '1') return false;
    const FormHooks hk = read_form_hooks();
    if (hk.no_tiled) return false;
    const int min_rows = hk.tiled_min_rows.set ? static_cast<int>(hk.tiled_min_rows.value) : 32 * kTileRows;
    // HPRLP_REORDER_ANYWAY=1 (test hook): the ordering at a small shape -- without the two gates a small matrix cannot pass (any
    // order of it fills its few 8192 x 2048 tiles: the tiling share is 1, and a tiled copy of the given order is valid already)
    const char *anyw = env_get("HPRLP_REORDER_ANYWAY");
    const bool anyway = anyw && anyw[0] == '1';
    if (comm || (A.view.tiled.valid && !anyway) || not_attempted_for_shape(A.outcome.why) || m < min_rows || n < min_rows) return false;
    const auto t0 = time_now();
    const sparseMatrix *As = model->A;
    const long nnz = As->numElements;
    ReorderStats st;
    // everything but the spectral ordering of the (small) cluster graph runs on the device, on the patterns of A and A^T
    // that are resident already; HPRLP_REORDER_HOST=1 keeps the clustering on the host (reorder.cpp, the reference form)
    const char *hostc = env_get("HPRLP_REORDER_HOST");
    const bool host_clusters = hostc && hostc[0] == '1';
    const bool timing = env_get("HPRLP_TIMING") != nullptr;
    auto tphase = time_now();
    auto tick = [&](const char *what) {
        if (timing) std::cerr << "[timing]   reorder " << what << " " << time_since(tphase) << " s" << std::endl;
        tphase = time_now();
    };
    st.fraction_before = device_tiling_dense_fraction(m, n, nnz, A.rowptr.p, A.col.p, nullptr, nullptr, stream);
    reorder_before = st.fraction_before;
    tick("tiling test (given order)");
    if (st.fraction_before >= 0.5 && !anyway) return false;  // the tiled build declined for another reason
    DBuf<double> dpr(static_cast<size_t>(m)), dpc(static_cast<size_t>(n));
    if (host_clusters) {
        std::vector<int> trp(static_cast<size_t>(n) + 1), tci(static_cast<size_t>(nnz));
        AT.rowptr.download(trp.data(), trp.size());
        AT.col.download(tci.data(), tci.size());
        std::vector<double> pr, pc;
        cluster_positions(m, n, As->rowPtr, As->colIndex, trp.data(), tci.data(), &pr, &pc, &st);
        dpr.upload(pr.data(), pr.size());
        dpc.upload(pc.data(), pc.size());
    } else {
        device_cluster_positions(m, n, nnz, A.rowptr.p, A.col.p, AT.rowptr.p, AT.col.p, dpr.p, dpc.p, &st, stream);
    }
    tick("clusters and their order");
    DBuf<int> d_r(static_cast<size_t>(m)), d_c(static_cast<size_t>(n));
    device_refine_order(m, n, A.rowptr.p, A.col.p, AT.rowptr.p, AT.col.p, dpr.p, dpc.p, kReorderSweeps, d_r.p, d_c.p, stream);
    tick("median sweeps");
    st.fraction_after = device_tiling_dense_fraction(m, n, nnz, A.rowptr.p, A.col.p, d_r.p, d_c.p, stream);
    reorder_after = st.fraction_after;
    tick("tiling test (permuted)");
    if (verbose || env_get("HPRLP_TIMING"))
        std::cerr << "[reorder] tiled share of the entries " << st.fraction_before << " -> " << st.fraction_after << " (" << st.clusters
                  << " clusters, " << st.components << " components, " << st.bfs_levels << " BFS levels, " << time_since(t0) << " s)" << std::endl;
    if (st.fraction_after < 0.5) {
        reorder_time = time_since(t0);
        return false;
    }
    std::vector<int> hr(static_cast<size_t>(m)), hc(static_cast<size_t>(n));
    d_r.download(hr.data(), hr.size());
    d_c.download(hc.data(), hc.size());
    // P A Q on the device, swapped into A
    DBuf<int> nrp(static_cast<size_t>(m) + 1), nci(static_cast<size_t>(nnz));
    DBuf<double> nval(static_cast<size_t>(nnz));
    device_permute_csr(m, n, nnz, A.rowptr.p, A.col.p, A.val.p, d_r.p, d_c.p, nrp.p, nci.p, nval.p, stream);
    src_rowptr = std::move(A.rowptr);  // the caller's pattern: what the value maps of set_matrix_values are built from
    src_col = std::move(A.col);
    A.rowptr = std::move(nrp);
    A.col = std::move(nci);
    A.val = std::move(nval);
    std::vector<int> hrp(static_cast<size_t>(m) + 1);
    A.rowptr.download(hrp.data(), hrp.size());
    // (under HPRLP_REORDER_ANYWAY a tiled copy of the given order may be in place: released here, describe() builds the permuted one)
    if (anyway) {
        A.tiled = DeviceTiled();
        A.view.tiled = TiledDev();
    }
    A.describe(m, n, hrp.data(), nullptr, nullptr);
    perm_r = std::move(hr);
    perm_c = std::move(hc);
    reorder_time = time_since(t0);
    return true;
}

void Solver::finish_tiling() {
    if (A.tiling.valid() || AT.tiling.valid()) {
        invalidate_far();
        // captured graphs (normal iterations, the power iteration's block of ten) bake in the kernel form of the views:
        // a view that is about to change from the stream kernel to its tiled copy makes them stale (slower, not wrong)
        for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
    if (A.tiling.valid()) A.finish_tiling(stream);
    if (AT.tiling.valid()) AT.finish_tiling(stream);
}

void Solver::setup_shard(int m_glob, int n_glob, int row_off_, int m_loc_, int col_off_, int n_loc_, const int *Arp,
                         const int *Aci, const double *Av, const int *ATrp, const int *ATci, const double *ATv,
                         const double *AL_, const double *AU_, const double *l_, const double *u_, const double *c_,
                         double obj_constant_, const HPRLP_parameters *param, Comm *comm_) {
    const auto t0 = time_now();
    prm = *param;
    comm = comm_;
    env_at_setup = env_in_effect(&env_ignored_at_setup);
    read_hooks();
    HIP_CHECK(hipSetDevice(prm.device_number));
    HIP_CHECK(hipStreamCreate(&stream));
    m = m_glob; n = n_glob;
    m_loc = m_loc_; n_loc = n_loc_;
    row_off = row_off_; col_off = col_off_;
    const int P = comm ? comm->size : 1;
    const int chunk_m = (m + P - 1) / P, chunk_n = (n + P - 1) / P;
    m_pad = chunk_m * P; n_pad = chunk_n * P;
    if (comm) {
        if (row_off != comm->rank * chunk_m || col_off != comm->rank * chunk_n ||
            m_loc != std::max(0, std::min(m, row_off + chunk_m) - row_off) ||
            n_loc != std::max(0, std::min(n, col_off + chunk_n) - col_off))
            throw std::runtime_error("shard bounds do not match the block partition of hprlp_partition()");
    }
    obj_constant = obj_constant_;
    A.upload(m_loc, n, Arp, Aci, Av);
    AT.upload(n_loc, m, ATrp, ATci, ATv);
    AL.alloc(m_loc); AL.upload(AL_, m_loc);
    AU.alloc(m_loc); AU.upload(AU_, m_loc);
    l.alloc(n_loc); l.upload(l_, n_loc);
    u.alloc(n_loc); u.upload(u_, n_loc);
    c.alloc(n_loc); c.upload(c_, n_loc);
    alloc_work();
    if (comm) {
        // length-m vectors are read through the columns of the A^T shard, length-n ones through those of A
        halo_m.build(comm, ATci, ATrp[n_loc], m, chunk_m, stream);
        halo_n.build(comm, Aci, Arp[m_loc], n, chunk_n, stream);
        verify_exchange();
    }
    finish_tiling();  // the shard arrays belong to the caller
    HIP_CHECK(hipDeviceSynchronize());
    setup_time = time_since(t0);
}

// ------------------------------------------------------------------------------------------------
// collectives (no-ops on one GPU)
// ------------------------------------------------------------------------------------------------
void HaloPlan::build(Comm *comm, const int *cols, long nnz, int total, int chunk, hipStream_t s) {
    const int P = comm->size, r = comm->rank;
    sparse = false;
    if (P <= 1) return;
    // entries of the gathered vector that this shard's column indices name, by owning rank
    std::vector<char> need(static_cast<size_t>(total), 0);
    for (long k = 0; k < nnz; ++k) need[cols[k]] = 1;
    std::vector<int> want;            // concatenated over peers, ascending inside a peer
    std::vector<long> want_off(P + 1, 0);
    for (int p = 0; p < P; ++p) {
        if (p != r) {
            const int lo = std::min(total, p * chunk), hi = std::min(total, (p + 1) * chunk);
            for (int j = lo; j < hi; ++j)
                if (need[j]) want.push_back(j);
        }
        want_off[p + 1] = static_cast<long>(want.size());
    }
    // request counts of everybody: cnt[a*P + b] = entries rank a wants from rank b
    std::vector<double> cnt(static_cast<size_t>(P) * P, 0.0);
    for (int p = 0; p < P; ++p) cnt[static_cast<size_t>(r) * P + p] = static_cast<double>(want_off[p + 1] - want_off[p]);
    DBuf<double> dcnt(static_cast<size_t>(P) * P);
    dcnt.upload(cnt.data(), cnt.size());
    comm->allgather_inplace(dcnt.p, static_cast<size_t>(P), s);
    HIP_CHECK(hipStreamSynchronize(s));
    dcnt.download(cnt.data(), cnt.size());
    total_requests = 0;
    for (double v : cnt) total_requests += static_cast<long>(v);
    const double dense = static_cast<double>(P - 1) * static_cast<double>(total);
    sparse = static_cast<double>(total_requests) <= 0.5 * dense;
    if (const char *e = env_get("HPRLP_DIST_EXCHANGE")) {  // "sparse" / "allgather": same value on every rank
        if (e[0] == 's') sparse = true;
        if (e[0] == 'a') sparse = false;
    }
    if (!sparse) return;

    nrecv = static_cast<int>(want.size());
    recv_idx.alloc(want.size());
    recv_idx.upload(want.data(), want.size());
    std::vector<long> send_off(P + 1, 0);
    for (int p = 0; p < P; ++p) send_off[p + 1] = send_off[p] + static_cast<long>(cnt[static_cast<size_t>(p) * P + r]);
    nsend = static_cast<int>(send_off[P]);
    send_idx.alloc(static_cast<size_t>(nsend));
    // tell every peer which of its entries we read (our request list becomes its send list)
    std::vector<P2P> idx_ops;
    for (int p = 0; p < P; ++p) {
        if (p == r) continue;
        const size_t nw = static_cast<size_t>(want_off[p + 1] - want_off[p]), ns = static_cast<size_t>(send_off[p + 1] - send_off[p]);
        if (nw || ns) idx_ops.push_back(P2P{p, recv_idx.p + want_off[p], nw * sizeof(int), send_idx.p + send_off[p], ns * sizeof(int)});
    }
    comm->exchange(idx_ops.data(), static_cast<int>(idx_ops.size()), s);
    HIP_CHECK(hipStreamSynchronize(s));
    {   // the kernels index without bounds checks: every requested entry must lie in our own slice
        std::vector<int> chk(static_cast<size_t>(nsend));
        send_idx.download(chk.data(), chk.size());
        const int lo = std::min(total, r * chunk), hi = std::min(total, (r + 1) * chunk);
        for (int v : chk)
            if (v < lo || v >= hi) throw std::runtime_error("halo plan: a peer requested an entry this rank does not own");
    }
    sendbuf.alloc_zero(static_cast<size_t>(nsend));
    recvbuf.alloc_zero(static_cast<size_t>(nrecv));
    ops.clear();
    for (int p = 0; p < P; ++p) {
        if (p == r) continue;
        const size_t nw = static_cast<size_t>(want_off[p + 1] - want_off[p]), ns = static_cast<size_t>(send_off[p + 1] - send_off[p]);
        if (nw || ns) ops.push_back(P2P{p, sendbuf.p + send_off[p], ns * sizeof(double), recvbuf.p + want_off[p], nw * sizeof(double)});
    }
}

void Solver::gather_on(double *gbuf, bool is_m, hipStream_t s) {
    if (!comm) return;  // (a one-rank communicator still runs the collective: used to test the RCCL path)
    // the exchange stream has its own communicator (one communicator, one stream)
    Comm *cm = (xcomm && comm_stream && s == comm_stream) ? xcomm : comm;
    HaloPlan &h = is_m ? halo_m : halo_n;
    if (!h.sparse) {
        const size_t chunk = static_cast<size_t>(is_m ? m_pad : n_pad) / cm->size;
        cm->allgather_inplace(gbuf, chunk, s);
        return;
    }
    launch_pack(gbuf, h.send_idx.p, h.sendbuf.p, h.nsend, s);
    cm->exchange(h.ops.data(), static_cast<int>(h.ops.size()), s);
    launch_scatter(gbuf, h.recv_idx.p, h.recvbuf.p, h.nrecv, s);
}

// One exchange of a vector whose entry j is j + 1 on its owner and -1 elsewhere: every entry this shard reads must
// arrive as j + 1.  All ranks agree on the outcome (all-reduce of the failure count); a neighbour exchange that fails
// is replaced by the all-gather on every rank, an all-gather that fails is an error.  Costs one exchange per vector
// length at set-up and keeps a transport problem from turning into silently wrong iterates.
void Solver::verify_exchange() {
    if (!comm || comm->size <= 1) return;
    const bool inject = env_get("HPRLP_DIST_SELFTEST_FAIL") != nullptr;  // tests: first verdict reads "failed"
    DBuf<double> flag(1);
    // with a second communicator both transports are tested: passes 0, 1 through comm on the solver stream, passes 2, 3
    // through xcomm on the exchange stream
    if (xcomm) ensure_comm_stream();
    for (int pass = 0; pass < (xcomm ? 4 : 2); ++pass) {
        const bool is_m = (pass & 1) == 0;
        hipStream_t vs = pass >= 2 ? comm_stream : stream;
        HaloPlan &h = is_m ? halo_m : halo_n;
        const int total = is_m ? m : n, pad = is_m ? m_pad : n_pad;
        const int chunk = pad / comm->size;
        const int lo = std::min(total, comm->rank * chunk), hi = std::min(total, (comm->rank + 1) * chunk);
        std::vector<double> init(static_cast<size_t>(pad), -1.0), got(static_cast<size_t>(pad));
        for (int j = lo; j < hi; ++j) init[j] = j + 1.0;
        DBuf<double> g(static_cast<size_t>(pad));
        for (int attempt = 0;; ++attempt) {
            g.upload(init.data(), init.size());
            gather_on(g.p, is_m, vs);
            HIP_CHECK(hipStreamSynchronize(vs));
            g.download(got.data(), got.size());
            double bad = 0.0;
            if (h.sparse) {
                std::vector<int> want(static_cast<size_t>(h.nrecv));
                h.recv_idx.download(want.data(), want.size());
                for (int j : want) bad += got[j] != j + 1.0;
                for (int j = lo; j < hi; ++j) bad += got[j] != j + 1.0;
                if (inject && attempt == 0) bad += 1.0;
            } else {
                for (int j = 0; j < total; ++j) bad += got[j] != j + 1.0;
            }
            flag.upload(&bad, 1);
            comm->allreduce_sum(flag.p, 1, stream);
            HIP_CHECK(hipStreamSynchronize(stream));
            flag.download(&bad, 1);
            if (bad == 0.0) break;
            if (!h.sparse || attempt > 0)
                throw std::runtime_error("multi-GPU exchange self-test failed: the all-gather did not deliver every rank's slice");
            if (comm->rank == 0)
                std::fprintf(stderr, "hprlp: neighbour exchange failed its self-test (%g wrong entries); using the all-gather\n", bad);
            h.sparse = false;
        }
    }
}

void Solver::fetch_enqueue() {
    const auto t0 = time_now();
    HIP_CHECK(hipMemcpyAsync(scal_h.p, scal.p, kNumScalars * sizeof(double), hipMemcpyDeviceToHost, stream));
    fetch_enqueue_s += time_since(t0);
}

void Solver::fetch_wait() {
    const auto t1 = time_now();
    HIP_CHECK(hipStreamSynchronize(stream));
    fetch_wait_s += time_since(t1);
    ++fetches;
}

void Solver::fetch_scalars() {
    fetch_enqueue();
    fetch_wait();
}

static void allreduce_slots(Solver *s, int first, int count) {
    if (!s->comm) return;
    s->comm->allreduce_sum(s->scal.p + first, count, s->stream);
}

double Solver::reduce_sum_sq(const double *v, int n_local) {
    launch_norm2(v, n_local, part_v.p, kReduceBlocks, stream);
    FinalizeArgs f{};
    f.n = 1;
    f.item[0] = {part_v.p, kReduceBlocks, S_TMP0};
    launch_finalize(f, scal.p, stream);
    allreduce_slots(this, S_TMP0, 1);
    fetch_scalars();
    return scal_h[S_TMP0];
}

static double bnorm_sq(Solver *s) {
    launch_bnorm2(s->AL.p, s->AU.p, s->m_loc, s->part_v.p, kReduceBlocks, s->stream);
    FinalizeArgs f{};
    f.n = 1;
    f.item[0] = {s->part_v.p, kReduceBlocks, S_TMP0};
    launch_finalize(f, s->scal.p, s->stream);
    allreduce_slots(s, S_TMP0, 1);
    s->fetch_scalars();
    return s->scal_h[S_TMP0];
}

// ------------------------------------------------------------------------------------------------
// scaling (reference src/scaling.cu:88-216).  t1 lives in the gathered m-vector gsm, t2 in gsn, so
// that the column-side scaling of each stored matrix can index the full vector.
// scale() is the sequence of the pieces below; scale_many (many.cpp) walks the same pieces for a group, recording into g.
// ------------------------------------------------------------------------------------------------
namespace {
// a scaling piece's launch: recorded for a group run, or issued on the member's stream
struct ScaleIssue {
    GroupLaunches *g;
    hipStream_t s;
    void zero(double *x, int n) const {  // (recorded: a fill of +0.0, the bits of the memset)
        if (g) g->fill(x, 0.0, n);
        else HIP_CHECK(hipMemsetAsync(x, 0, sizeof(double) * n, s));
    }
    void fill(double *x, double a, int n) const { g ? g->fill(x, a, n) : launch_fill(x, a, n, s); }
    void vec_scale(double *x, const double *v, int n, bool divide) const { g ? g->vec_scale(x, v, n, divide) : launch_vec_scale(x, v, n, divide, s); }
    void vec_scal(double *x, double a, int n) const { g ? g->vec_scal(x, a, n) : launch_vec_scal(x, a, n, s); }
    void exp_clamp(double *v, int n) const { g ? g->exp_clamp(v, n) : launch_exp_clamp(v, n, s); }
    void row_norm(const CsrDev &M, double *result, int norm) const { g ? g->row_norm(M, result, norm) : launch_row_norm(M, result, norm, s); }
    void scale_matrix(const CsrDev &M, const double *rowvec, const double *colvec_full, bool row_first, bool divide, double *next) const {
        g ? g->scale_matrix(M, rowvec, colvec_full, row_first, divide, next) : launch_scale_matrix(M, rowvec, colvec_full, row_first, divide, s, next);
    }
};
}  // namespace

// Alone the two sums share part_v and S_TMP0, with a host round trip between them.  Recorded, the second reduction has the upper
// half of part_v for its partials (2 x kReduceBlocks are allocated) and both sums are finalised into the caller's two slots --
// where a partial or a sum is stored does not change its value; also_tmp0: |c|^2 into S_TMP0 too, where the member's own last
// reduction leaves it.
void Solver::scale_sums(ScaleWalk *w, GroupLaunches *g, double out[2], bool also_tmp0) {
    if (!g) {
        out[0] = bnorm_sq(this);
        out[1] = reduce_sum_sq(c.p, n_loc);
        return;
    }
    g->bnorm2(AL.p, AU.p, m_loc, part_v.p);
    g->norm2(c.p, n_loc, part_v.p + kReduceBlocks);
    FinalizeArgs f{};
    f.n = 2;
    f.item[0] = {part_v.p, kReduceBlocks, 0};
    f.item[1] = {part_v.p + kReduceBlocks, kReduceBlocks, 1};
    g->finalize(f, w->sums);
    f.n = 1;
    f.item[0] = {part_v.p + kReduceBlocks, kReduceBlocks, S_TMP0};
    if (also_tmp0) g->finalize(f, scal.p);
}
void Solver::scale_norms_org(const double sums[2]) {
    norm_b_org = 1.0 + std::sqrt(sums[0]);
    norm_c_org = 1.0 + std::sqrt(sums[1]);
}
void Solver::scale_norms(const double sums[2]) {
    norm_b = std::sqrt(sums[0]);
    norm_c = std::sqrt(sums[1]);
}

void Solver::scale_begin(ScaleWalk *w, GroupLaunches *g) {
    const ScaleIssue on{g, stream};
    invalidate_far();
    overlap_ready = false;  // the split copies of the shards carry matrix values
    ovA.reset();
    ovAT.reset();
    // Every matrix-scaling pass that a Ruiz pass follows also leaves that pass's row norms (max |a| of the scaled rows, kernels.hip:
    // k_scale_matrix<.., NEXT>) in a second pair of gathered vectors, so the norm passes over the matrices are not run; the pairs
    // change roles pass by pass.  HPRLP_NO_FUSED_NORMS=1: separate norm passes (A/B runs, tests).
    w->fuse = prm.use_Ruiz_scaling && env_get("HPRLP_NO_FUSED_NORMS") == nullptr;
    if (w->fuse) {
        if (!g) {
            w->gsm2.alloc(static_cast<size_t>(m_pad));
            w->gsn2.alloc(static_cast<size_t>(n_pad));
            w->gm_next = w->gsm2.p, w->gn_next = w->gsn2.p;
        }
        on.zero(w->gm_next, m_pad);
        on.zero(w->gn_next, n_pad);
    }
    w->gm = gsm.p, w->gn = gsn.p;
    w->have_norms = false;
    w->passes = (prm.use_Ruiz_scaling ? 10 : 0) + (prm.use_Pock_Chambolle_scaling ? 1 : 0);
    on.fill(row_norm.p, 1.0, m_loc);
    on.fill(col_norm.p, 1.0, n_loc);
    double sums[2];
    scale_sums(w, g, sums);
    if (!g) scale_norms_org(sums);
    if (!prm.use_CR_scaling) return;  // :40-83
    on.zero(gsm.p, m_pad);
    on.zero(gsn.p, n_pad);
    if (g) return;  // (the matrices of a group launch have no tiled copy)
    // Matrices with a tiled copy run the 40 passes through the tiled kernel on a second value array of the copy that
    // holds -log|a| (formed once; released when the passes are done).  HPRLP_NO_TILED_CR=1: stream kernel (A/B runs).
    finish_tiling();
    const bool tiled_cr = env_get("HPRLP_NO_TILED_CR") == nullptr;
    auto log_values = [&](DeviceMatrix &M, DBuf<double> &tile, DBuf<double> &far) {
        if (!tiled_cr || !cr_runs_tiled(M.view)) return;
        tile.alloc(static_cast<size_t>(std::max<long>(M.tiled.n_tile, 1)));
        far.alloc(static_cast<size_t>(std::max<long>(M.tiled.n_rem, 1)));
        launch_tiled_refresh_log(M.tiled, M.val.p, tile.p, far.p, stream);
    };
    log_values(A, w->logA_tile, w->logA_far);
    log_values(AT, w->logAT_tile, w->logAT_far);
}

void Solver::scale_cr_sweep(ScaleWalk *w, bool transposed, GroupLaunches *g) {
    DeviceMatrix &M = transposed ? AT : A;
    const double *other = transposed ? gsm.p : gsn.p;
    double *result = transposed ? gsn.p + col_off : gsm.p + row_off;
    if (g) return g->cr_log_update(M.view, other, result);
    launch_cr_log_update(M.view, other, result, stream, transposed ? w->logAT_tile.p : w->logA_tile.p, transposed ? w->logAT_far.p : w->logA_far.p);
    gather(transposed ? gsn.p : gsm.p, !transposed);
}

void Solver::scale_cr_exp(ScaleWalk *w, GroupLaunches *g) {
    const ScaleIssue on{g, stream};
    if (w->logA_tile.p || w->logAT_tile.p) HIP_CHECK(hipStreamSynchronize(stream));  // the log values are released after the scaling pass
    on.exp_clamp(gsm.p + row_off, m_loc);
    on.exp_clamp(gsn.p + col_off, n_loc);
    gather(gsm.p, true);
    gather(gsn.p, false);
}

void Solver::scale_cr_apply(ScaleWalk *w, GroupLaunches *g) {
    const ScaleIssue on{g, stream};
    double *t1 = gsm.p + row_off, *t2 = gsn.p + col_off;
    const bool max_next = w->fuse;  // (a CR scaling pass is followed by Ruiz pass 0)
    on.vec_scale(row_norm.p, t1, m_loc, true);
    on.vec_scale(col_norm.p, t2, n_loc, true);
    on.scale_matrix(A.view, t1, gsn.p, /*row_first=*/true, /*divide=*/false, max_next ? w->gm_next + row_off : nullptr);
    on.scale_matrix(AT.view, t2, gsm.p, /*row_first=*/false, /*divide=*/false, max_next ? w->gn_next + col_off : nullptr);
    w->have_norms = max_next;
    on.vec_scale(AL.p, t1, m_loc, false);
    on.vec_scale(AU.p, t1, m_loc, false);
    on.vec_scale(c.p, t2, n_loc, false);
    on.vec_scale(l.p, t2, n_loc, true);
    on.vec_scale(u.p, t2, n_loc, true);
    w->logAT_far.release(), w->logAT_tile.release(), w->logA_far.release(), w->logA_tile.release();
}

void Solver::scale_pass(ScaleWalk *w, int it, GroupLaunches *g) {  // Ruiz :123-153 then Pock-Chambolle :157-183
    if (it >= w->passes) return;
    const ScaleIssue on{g, stream};
    const int norm = (prm.use_Ruiz_scaling && it < 10) ? 99 : 1;
    if (w->have_norms) {  // left by the previous scaling pass in the other pair of vectors
        std::swap(w->gm, w->gm_next);
        std::swap(w->gn, w->gn_next);
    }
    double *t1 = w->gm + row_off, *t2 = w->gn + col_off;
    if (!w->have_norms) {
        on.row_norm(A.view, t1, norm);
        on.row_norm(AT.view, t2, norm);
    }
    gather(w->gm, true);
    gather(w->gn, false);
    on.vec_scale(row_norm.p, t1, m_loc, false);
    on.vec_scale(AL.p, t1, m_loc, true);
    on.vec_scale(AU.p, t1, m_loc, true);
    on.vec_scale(col_norm.p, t2, n_loc, false);
    const bool next = w->fuse && it + 1 < w->passes && it + 1 < 10;  // a max-norm (Ruiz) pass follows
    on.scale_matrix(A.view, t1, w->gn, true, true, next ? w->gm_next + row_off : nullptr);
    on.scale_matrix(AT.view, t2, w->gm, false, true, next ? w->gn_next + col_off : nullptr);
    w->have_norms = next;
    on.vec_scale(c.p, t2, n_loc, true);
    on.vec_scale(l.p, t2, n_loc, false);
    on.vec_scale(u.p, t2, n_loc, false);
}

void Solver::scale_bc_apply(const double sums[2], GroupLaunches *g) {  // :185-202
    if (!prm.use_bc_scaling) {
        b_scale = 1.0;
        c_scale = 1.0;
        return;
    }
    const ScaleIssue on{g, stream};
    b_scale = 1.0 + std::sqrt(sums[0]);
    c_scale = 1.0 + std::sqrt(sums[1]);
    const double bs = 1.0 / b_scale, cs = 1.0 / c_scale;
    on.vec_scal(AU.p, bs, m_loc);
    on.vec_scal(AL.p, bs, m_loc);
    on.vec_scal(l.p, bs, n_loc);
    on.vec_scal(u.p, bs, n_loc);
    on.vec_scal(c.p, cs, n_loc);
}

void Solver::scale_finish(ScaleWalk *w, GroupLaunches *g, double out[2]) {
    scale_sums(w, g, out, /*also_tmp0=*/true);
    if (!g) scale_norms(out);
    finish_tiling();  // tiled copies still being built pick up the scaled values here ...
    A.refresh_tiled(stream);  // ... finished ones are refreshed
    AT.refresh_tiled(stream);
    refresh_bound_codes(g);
}

void Solver::scale_end(GroupLaunches *g) {  // (the gathered vectors were a pass's scale vectors: zeroed after everything that read them)
    const ScaleIssue on{g, stream};
    on.zero(gsm.p, m_pad);
    on.zero(gsn.p, n_pad);
}

void Solver::scale() {
    const auto t0 = time_now();
    ScaleWalk w;
    double sums[2];
    scale_begin(&w);
    if (prm.use_CR_scaling) {
        for (int it = 0; it < 20; ++it) {
            scale_cr_sweep(&w, false);
            scale_cr_sweep(&w, true);
        }
        scale_cr_exp(&w);
        scale_cr_apply(&w);
    }
    for (int it = 0; it < w.passes; ++it) scale_pass(&w, it);
    if (prm.use_bc_scaling) scale_sums(&w, nullptr, sums);
    scale_bc_apply(sums);
    scale_finish(&w, nullptr, sums);
    scale_end();
    HIP_CHECK(hipStreamSynchronize(stream));
    scaling_time = time_since(t0);
    scaled = true;
}

// ------------------------------------------------------------------------------------------------
// lambda_max(A A^T) by the power method (reference src/power_iteration.cu:20-119).  q lives in gsm,
// A^T q in gsn, z in sm1; the dots ride on the second SpMV's epilogue and stay on the device; the
// host reads back only at the every-10th-iteration convergence check.
// ------------------------------------------------------------------------------------------------
SmallArgs Solver::small_args() const {
    return SmallArgs{m, n, A.view.nnz, A.view.rowptr, AT.view.rowptr, AT.view.val, small_ij.p, small_posA.p,
                     small_order_x.p, small_order_y.p, x.p, x_hat, y, l.p, u.p, c.p, last_x.p, AL.p, AU.p, last_y.p, ctrl.p};
}

bool Solver::small_power_wanted() const {
    const bool no_small_power = env_get("HPRLP_NO_SMALL_POWER") != nullptr;  // tests: the regular kernels instead
    return use_small && !comm && !no_small_power;
}

void Solver::power_start(double *z) {
    // large vectors in the caller's numbering are filled on the device (last-place differences from the host's libm are
    // possible there; below the threshold the start vector is the oracle's bit for bit)
    const bool host_start = env_get("HPRLP_HOST_POWER_START") != nullptr;  // (tests)
    if (m_loc > kDeviceStartRows && perm_r.empty() && !host_start) {
        launch_pw_start(m_loc, 1ULL, row_off, z, stream);
    } else {
        std::vector<double> z0(static_cast<size_t>(std::max(m_loc, 1)));
        power_start_vector(m_loc, 1ULL, row_off, z0.data());
        if (!perm_r.empty()) {  // the start vector is defined in the caller's row numbering
            std::vector<double> zp(z0.size());
            for (int i = 0; i < m_loc; ++i) zp[i] = z0[perm_r[i]];
            z0.swap(zp);
        }
        HIP_CHECK(hipMemcpyAsync(z, z0.data(), sizeof(double) * m_loc, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
}

// The pieces of the regular path: z in sm1, q in gsm, A^T q in gsn.  g records them for the group launches of wide members
// (many.cpp: power_iteration_many), which have neither a tiled copy nor an exchange: no hand-off, no gather, no all-reduce.
void Solver::power_norm(GroupLaunches *g) {
    double *z = sm1.p;
    FinalizeArgs f0{};
    f0.n = 1;
    f0.item[0] = {part_v.p, kReduceBlocks, S_PW_ZZ};
    if (g) {
        g->norm2(z, m_loc, part_v.p);
        g->finalize(f0, scal.p);
        return;
    }
    launch_norm2(z, m_loc, part_v.p, kReduceBlocks, stream);
    launch_finalize(f0, scal.p, stream);
    allreduce_slots(this, S_PW_ZZ, 1);
}

bool Solver::power_piece(int piece, GroupLaunches *g, bool handed) {
    double *q = gsm.p + row_off, *ATq = gsn.p + col_off, *z = sm1.p;
    if (piece == 0) {
        if (g) {
            g->pw_normalize(z, q, m_loc, scal.p);
            return false;
        }
        launch_pw_normalize(z, q, m_loc, scal.p, stream);
        gather(gsm.p, true);
        return false;
    }
    if (piece == 1) {
        if (g) {
            g->spmv_push(AT.view, gsm.p, ATq);
            return false;
        }
        // A^T q: its epilogue writes the products A's remainder needs (hand-off, as between the half-steps; A then runs without a
        // pre-pass) -- where the remainder is a large part of A.  With a few per cent of the entries in it the pre-pass is the
        // cheaper way since round 4: config 5 (5 %), same box: push 104 us of the launch against 64 us of k_far_products, power
        // iteration 0.385 -> 0.374 s
        const bool push_pays = A.view.tiled.valid && static_cast<double>(A.tiled.n_rem) >= 0.3 * static_cast<double>(A.view.nnz);
        const bool h = launch_spmv_push(AT.view, gsm.p, ATq, push_pays ? push_into(A, AT) : FarPush{}, stream);
        gather(gsn.p, false);
        return h;
    }
    const int gridA = A.view.grid();
    FinalizeArgs f{};
    f.n = 2;
    f.item[0] = {part_y.p, gridA, S_PW_ZZ};
    f.item[1] = {part_y.p + stride_y, gridA, S_PW_QZ};
    if (g) {
        g->spmv_dots(A.view, gsn.p, z, q, part_y.p, stride_y);
        g->finalize(f, scal.p);
        return false;
    }
    launch_spmv_plain(A.view, gsn.p, z, q, true, part_y.p, stride_y, stream, handed);
    launch_finalize(f, scal.p, stream);
    allreduce_slots(this, S_PW_ZZ, 2);
    return false;
}

void Solver::power_err(GroupLaunches *g) {
    double *q = gsm.p + row_off, *z = sm1.p;
    FinalizeArgs fe{};
    fe.n = 1;
    fe.item[0] = {part_v.p, kReduceBlocks, S_PW_ERR2};
    if (g) {
        g->pw_err(z, q, m_loc, scal.p, part_v.p);
        g->finalize(fe, scal.p);
        return;
    }
    launch_pw_err(z, q, m_loc, scal.p, part_v.p, kReduceBlocks, stream);
    launch_finalize(fe, scal.p, stream);
    allreduce_slots(this, S_PW_ERR2, 1);
}

double Solver::power_iteration(int max_iter, double tol, int *iters) {
    finish_tiling();
    invalidate_far();
    const auto t0 = time_now();
    double *z = sm1.p;  // (q in gsm, A^T q in gsn: the pieces below)
    power_start(z);
    if (small_power_wanted()) {
        // Netlib-scale LP: the whole power iteration in one launch of the single-workgroup kernel (small.hip), stopping test on
        // the device; the host waits once
        const SmallArgs a = small_args();
        HIP_CHECK(hipMemsetAsync(scal.p + S_SMALL_PW_LAMBDA, 0, 2 * sizeof(double), stream));
        launch_small_power(a, z, max_iter, tol, scal.p + S_SMALL_PW_LAMBDA, stream);
        fetch_scalars();
        const double lambda_dev = scal_h[S_SMALL_PW_LAMBDA];
        const int done_dev = static_cast<int>(scal_h[S_SMALL_PW_ITERS]);
        // a kernel that did not run leaves the zeroed slots; a lambda that is not a positive finite number is no eigenvalue
        // estimate either: the regular kernels below take over (same start vector, still in z)
        if (done_dev > 0 && std::isfinite(lambda_dev) && lambda_dev > 0.0) {
            if (iters) *iters = done_dev;
            power_iters = done_dev;
            power_time = time_since(t0);
            return lambda_dev;
        }
        if (verbose) std::cerr << "[hprlp] single-launch power iteration returned lambda = " << lambda_dev << " after " << done_dev
                               << " iterations: falling back to the regular kernels" << std::endl;
    }
    power_norm();

    double lambda = 1.0;
    int done = max_iter;
    auto one_iteration = [&]() {
        power_piece(0);
        const bool handed = power_piece(1);
        power_piece(2, nullptr, handed);
    };
    auto error_terms = [&]() { power_err(); };
    // One rank: the ten iterations between two stopping tests are one graph launch (about 50 kernels; enqueued one by one the
    // launches of config 5 leave 0.2 ms of every 1.45 ms iteration idle, on config 3 the iteration is launch-bound altogether).
    hipGraphExec_t block = nullptr;
    if (use_graph && max_iter >= 10) {
        auto it = graphs.find(kPowerBlockKey);
        if (it != graphs.end()) {
            block = it->second;
        } else {
            hipGraph_t g = nullptr;
            HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            for (int k = 0; k < 10; ++k) one_iteration();
            error_terms();
            HIP_CHECK(hipStreamEndCapture(stream, &g));
            HIP_CHECK(hipGraphInstantiate(&block, g, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphDestroy(g));
            graphs[kPowerBlockKey] = block;
        }
    }
    for (int i = 1; i <= max_iter; ++i) {
        if (block && i % 10 == 1 && i + 9 <= max_iter) {
            HIP_CHECK(hipGraphLaunch(block, stream));
            i += 9;
        } else {
            one_iteration();
            if (i % 10 == 0) error_terms();
        }
        if (i % 10 == 0) {
            fetch_scalars();
            lambda = scal_h[S_PW_QZ];
            const double err = std::sqrt(scal_h[S_PW_ERR2]);
            if (err < tol) {
                done = i;
                break;
            }
        }
    }
    if (iters) *iters = done;
    power_iters = done;
    // leave the scratch vectors clean
    HIP_CHECK(hipMemsetAsync(gsm.p, 0, sizeof(double) * m_pad, stream));
    HIP_CHECK(hipMemsetAsync(gsn.p, 0, sizeof(double) * n_pad, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    power_time = time_since(t0);
    return lambda;
}

// ------------------------------------------------------------------------------------------------
void Solver::set_sigma_lambda(double sigma_, double lambda_, bool reset_k, GroupLaunches *g) {
    sigma = sigma_;
    lambda_max = lambda_;
    if (g) g->set_ctrl(ctrl.p, sigma, lambda_max, reset_k ? 1 : 0);
    else launch_set_ctrl(ctrl.p, sigma, lambda_max, reset_k ? 1 : 0, stream);
}

bool Solver::joins_group() {
    if (!(use_small || group_wide) || comm) return false;
    finish_tiling();
    return group_form_fits(A.view) && group_form_fits(AT.view);
}

// hooks that the iteration path consults: read when the solver is set up (a later change of the environment does not reach it)
void Solver::read_hooks() {
    hook_no_far_push = env_get("HPRLP_NO_FAR_PUSH") && env_get("HPRLP_NO_FAR_PUSH")[0] == '1';
    hook_no_bound_codes = env_get("HPRLP_NO_BOUND_CODES") != nullptr;  // A/B runs: always read l and u
    hook_store_x = env_get("HPRLP_STORE_X") != nullptr;                // A/B runs: every x-half reads and stores x
}

void Solver::refresh_bound_codes(GroupLaunches *g) {
    if (hook_no_bound_codes) return;
    if (n_loc > 0) {
        if (lu_code.n != static_cast<size_t>(n_loc)) lu_code.alloc(static_cast<size_t>(n_loc));
        if (g) g->bound_codes(n_loc, l.p, u.p, lu_code.p);
        else launch_bound_codes(n_loc, l.p, u.p, lu_code.p, stream);
    }
    if (m_loc > 0) {
        if (row_code.n != static_cast<size_t>(m_loc)) row_code.alloc(static_cast<size_t>(m_loc));
        if (g) g->row_codes(m_loc, AL.p, AU.p, row_code.p);
        else launch_row_codes(m_loc, AL.p, AU.p, row_code.p, stream);
    }
}

bool Solver::bound_codes_in_place() const {
    return hook_no_bound_codes || (row_code.n == static_cast<size_t>(m_loc) && lu_code.n == static_cast<size_t>(n_loc));
}

bool Solver::joins_group_resolve() {
    return joins_group() && perm_r.empty() && perm_c.empty() && bound_codes_in_place() && !y_exchange_pending && !overlap_enabled;
}

// Back to the state of a fresh solver after scale() and power_iteration(): every iterate and work vector zero, nothing handed over.
// (bench.py: the timed iterations and the solve to tolerance of a multi-GPU run use ONE solver -- a second one would need a
// second set of communicators.)  Call init_iteration_state() / set_sigma_lambda() afterwards, as after create.
void Solver::reset_iterates(GroupLaunches *g) {
    if (y_exchange_pending) throw std::runtime_error("reset_iterates: an exchange is still pending");
    invalidate_far();
    static_assert(sizeof(Ctrl) % sizeof(double) == 0, "the group's zeroing fills Ctrl as doubles (+0.0: all bits zero)");
    // (g: fill tasks of +0.0, the bits of the memsets; the group's launch and wait are the caller's)
    auto zero = [&](double *p, size_t n) {
        if (!(p && n > 0)) return;
        if (g) g->fill(p, 0.0, static_cast<int>(n));
        else HIP_CHECK(hipMemsetAsync(p, 0, sizeof(double) * n, stream));
    };
    zero(x.p, x.n); zero(last_x.p, last_x.n); zero(z_bar.p, z_bar.n);
    zero(last_y.p, last_y.n); zero(y_obj.p, y_obj.n); zero(y_temp.p, y_temp.n);
    zero(gy.p, gy.n); zero(gyb.p, gyb.n); zero(gsm.p, gsm.n);
    zero(gxh.p, gxh.n); zero(gxb.p, gxb.n); zero(gxt.p, gxt.n); zero(gsn.p, gsn.n);
    zero(sm1.p, sm1.n); zero(sn1.p, sn1.n);
    zero(scal.p, scal.n);
    if (g) {
        g->fill(reinterpret_cast<double *>(ctrl.p), 0.0, static_cast<int>(sizeof(Ctrl) / sizeof(double)));
        return;
    }
    HIP_CHECK(hipMemsetAsync(ctrl.p, 0, sizeof(Ctrl), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// g: the bound codes and ctrl recorded; sigma_ > 0 (g only) takes the place of the rule's sigma -- alone the override is a second
// k_set_ctrl that overwrites every word the first one wrote, so one task with the final sigma leaves the same bits
void Solver::init_iteration_state(GroupLaunches *g, double sigma_) {  // reference src/HPRLP.cu:154-167
    finish_tiling();
    invalidate_far();
    refresh_bound_codes(g);
    if (overlap_enabled && !overlap_ready) prepare_overlap();  // set-up work, not part of the first iteration
    const double s0 = (norm_b > 1e-8 && norm_c > 1e-8) ? norm_b / norm_c : 1.0;
    set_sigma_lambda(g && sigma_ > 0.0 ? sigma_ : s0, lambda_max, true, g);
}

// Column split of one shard on the device: local = entries whose column lies in [lo, hi).
static void split_shard(const DeviceMatrix &M, int lo, int hi, Solver::SplitShard *out, hipStream_t s) {
    const int rows = M.view.rows, cols = M.view.cols;
    device_split_columns(rows, M.view.nnz, M.rowptr.p, M.col.p, M.val.p, lo, hi, out->loc.rowptr, out->loc.col, out->loc.val,
                         out->rem.rowptr, out->rem.col, out->rem.val, s);
    std::vector<int> rp(static_cast<size_t>(rows) + 1);
    out->loc.rowptr.download(rp.data(), rp.size());
    out->loc.describe(rows, cols, rp.data(), nullptr, nullptr);
    out->rem.rowptr.download(rp.data(), rp.size());
    out->rem.describe(rows, cols, rp.data(), nullptr, nullptr);
    out->loc.finish_tiling(s);
    out->rem.finish_tiling(s);
    out->part.alloc_zero(static_cast<size_t>(std::max(rows, 1)));
    // The local part runs BESIDE the exchange's kernels.  The persistent schedule of the tiled kernel assumes that all
    // of its workgroups are resident; a CU that also hosts a workgroup of the exchange would leave one of them waiting
    // for a whole cohort list.  One workgroup per super-block (dispatched as slots free up) has no such tail.
    if (out->loc.view.tiled.valid) out->loc.view.tiled.grid = 8 * out->loc.view.tiled.per;
}

void Solver::ensure_comm_stream() {
    if (!comm_stream) {
        // highest priority: the few workgroups of the exchange must not queue behind the half-step's grid
        int prio_low = 0, prio_high = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        HIP_CHECK(hipStreamCreateWithPriority(&comm_stream, hipStreamDefault, prio_high));
        HIP_CHECK(hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_done_x, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_done_y, hipEventDisableTiming));
    }
}

void Solver::prepare_overlap() {
    finish_tiling();
    HIP_CHECK(hipStreamSynchronize(stream));
    ensure_comm_stream();
    ovAT.reset(new SplitShard);  // A^T shard: n_loc rows, columns = rows of A; this rank owns y[row_off, row_off + m_loc)
    split_shard(AT, row_off, row_off + m_loc, ovAT.get(), stream);
    ovA.reset(new SplitShard);   // A shard: m_loc rows; this rank owns x_hat[col_off, col_off + n_loc)
    split_shard(A, col_off, col_off + n_loc, ovA.get(), stream);
    HIP_CHECK(hipDeviceSynchronize());
    overlap_ready = true;
}

// The hand-off needs the PRODUCER to run the fused tiled kernel on one GPU (a super-block's rows = one source group of
// the consumer's remainder) and the consumer to have remainder lists; HPRLP_NO_FAR_PUSH=1 keeps the pre-pass (A/B runs).
FarPush Solver::push_into(const DeviceMatrix &consumer, const DeviceMatrix &producer) const {
    const TiledDev &pt = producer.view.tiled;
    if (hook_no_far_push || comm || !pt.valid || pt.n_pieces > 0) return FarPush{};
    if (consumer.view.tiled.valid && consumer.view.tiled.G != pt.R) return FarPush{};  // a source group must be ONE super-block of the producer
    return far_push_of(consumer.view);
}

int Solver::x_mode_of(int i, int count) const {
    if (hook_store_x || overlap_enabled || !AT.view.tiled.valid) return 0;
    return (i > 0 ? kXRebuild : 0) | (i + 1 < count ? kXNoStore : 0);
}

XHalfArgs Solver::normal_x_args(int x_mode) {
    XHalfArgs xa{gy.p, x.p, x_hat, l.p, u.p, c.p, last_x.p, nullptr, nullptr, nullptr, ctrl.p, nullptr, 0};
    xa.lu_code = lu_code.p;
    xa.x_mode = x_mode;
    return xa;
}

YHalfArgs Solver::normal_y_args() {
    YHalfArgs ya{gxh.p, y, AL.p, AU.p, last_y.p, nullptr, nullptr, nullptr, ctrl.p, nullptr, 0};  // (push / far_ready: the caller's)
    ya.row_code = row_code.p;
    return ya;
}

// (a wide member has neither tiled copies nor an exchange: x_mode_of gives 0, push_into nothing, the gathers do nothing)
void Solver::normal_half(bool y_half, GroupLaunches &g) {
    if (y_half) g.y_half(A.view, normal_y_args());
    else g.x_half(AT.view, normal_x_args(0));
}

void Solver::launch_normal_pair(bool more_follow, hipEvent_t *ev, int x_mode) {
    XHalfArgs xa = normal_x_args(x_mode);
    YHalfArgs ya = normal_y_args();
    if (ev) HIP_CHECK(hipEventRecord(ev[0], stream));
    if (!overlap_enabled) {
        xa.push = push_into(A, AT);
        xa.far_ready = far_AT_ready;
        far_A_ready = launch_x_half(AT.view, xa, false, stream);
        if (ev) HIP_CHECK(hipEventRecord(ev[1], stream));
        gather(gxh.p, false);
        ya.push = push_into(AT, A);
        ya.far_ready = far_A_ready;
        far_AT_ready = launch_y_half(A.view, ya, false, stream);
        if (ev) HIP_CHECK(hipEventRecord(ev[2], stream));
        gather(gy.p, true);
        return;
    }
    invalidate_far();
    if (!overlap_ready) prepare_overlap();
    // Exchange on comm_stream behind ev_ready, beside the local-column SpMV on the solver stream.  RCCL only enqueues,
    // so the exchange goes first and its workgroups are placed before the SpMV's grid fills the chip; the in-process
    // group blocks the host inside the exchange, so there the SpMV is launched first to run beside it.
    auto exchange_beside = [&](double *gbuf, bool is_m, hipEvent_t done, const CsrDev *local, double *part) {
        HIP_CHECK(hipEventRecord(ev_ready, stream));
        const bool spmv_first = overlap_spmv_first;
        if (local && spmv_first) launch_spmv_plain(*local, gbuf, part, nullptr, false, nullptr, 0, stream);
        HIP_CHECK(hipStreamWaitEvent(comm_stream, ev_ready, 0));
        gather_on(gbuf, is_m, comm_stream);
        HIP_CHECK(hipEventRecord(done, comm_stream));
        if (local && !spmv_first) launch_spmv_plain(*local, gbuf, part, nullptr, false, nullptr, 0, stream);
    };
    // ---- x-half: if the exchange of y is still in flight, the local-column part runs beside it
    if (y_exchange_pending) {
        if (!overlap_spmv_first)  // (the in-process group launched it before its blocking exchange, below)
            launch_spmv_plain(ovAT->loc.view, gy.p, ovAT->part.p, nullptr, false, nullptr, 0, stream);
        HIP_CHECK(hipStreamWaitEvent(stream, ev_done_y, 0));
        launch_x_half_base(ovAT->rem.view, xa, ovAT->part.p, stream);
        y_exchange_pending = false;
    } else {
        launch_x_half(AT.view, xa, false, stream);  // gathered y complete: the unsplit shard in one launch
    }
    if (ev) HIP_CHECK(hipEventRecord(ev[1], stream));
    // ---- exchange of x_hat beside the local-column part of the y-half
    exchange_beside(gxh.p, false, ev_done_x, &ovA->loc.view, ovA->part.p);
    HIP_CHECK(hipStreamWaitEvent(stream, ev_done_x, 0));
    launch_y_half_base(ovA->rem.view, ya, ovA->part.p, stream);
    if (ev) HIP_CHECK(hipEventRecord(ev[2], stream));
    // ---- exchange of y: beside the local-column part of the next pair's x-half, or waited for
    exchange_beside(gy.p, true, ev_done_y, more_follow && overlap_spmv_first ? &ovAT->loc.view : nullptr, ovAT->part.p);
    if (more_follow) y_exchange_pending = true;
    else HIP_CHECK(hipStreamWaitEvent(stream, ev_done_y, 0));
}

void Solver::step(bool check, GroupLaunches *g) {
    finish_tiling();
    if (!check) {
        launch_normal_pair();
        return;
    }
    XHalfArgs xa{gy.p, x.p, x_hat, l.p, u.p, c.p, last_x.p, x_bar, z_bar.p, x_temp, ctrl.p, part_x.p, stride_x};
    xa.lu_code = lu_code.p;
    xa.push = push_into(A, AT);
    xa.far_ready = far_AT_ready;
    if (g) g->x_half_check(AT.view, xa);  // (a member of the group launches has neither tiled copies nor an exchange)
    else far_A_ready = launch_x_half(AT.view, xa, true, stream);
    gather(gxh.p, false);
    YHalfArgs ya{gxh.p, y, AL.p, AU.p, last_y.p, y_bar, y_obj.p, y_temp.p, ctrl.p, part_y.p, stride_y};
    ya.row_code = row_code.p;
    ya.push = push_into(AT, A);
    ya.far_ready = far_A_ready;
    if (g) g->y_half_check(A.view, ya);
    else far_AT_ready = launch_y_half(A.view, ya, true, stream);
    gather(gy.p, true);
    FinalizeArgs f{};
    const int gx = AT.view.grid(), gyy = A.view.grid();
    f.n = 5;
    f.item[0] = {part_x.p, gx, S_CX};
    f.item[1] = {part_x.p + stride_x, gx, S_XZ};
    f.item[2] = {part_x.p + 2 * static_cast<size_t>(stride_x), gx, S_DX2};
    f.item[3] = {part_y.p, gyy, S_YOBJ_Y};
    f.item[4] = {part_y.p + stride_y, gyy, S_DY2};
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
}

hipGraphExec_t Solver::graph_for(int len) {
    auto it = graphs.find(len);
    if (it != graphs.end()) return it->second;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    // a replayed graph cannot look at the hand-off flags: it always starts with the pre-pass of A^T (as if nothing had been
    // handed over) and ends with both buffers handed over, whatever ran before it
    far_AT_ready = false;
    HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < len; ++i) launch_normal_pair(false, nullptr, x_mode_of(i, len));
    HIP_CHECK(hipStreamEndCapture(stream, &g));
    graph_end_A = far_A_ready;
    graph_end_AT = far_AT_ready;
    invalidate_far();  // nothing has run yet
    HIP_CHECK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(g));
    graphs[len] = ge;
    return ge;
}

void Solver::run_normal(int count) {
    if (count <= 0) return;
    finish_tiling();
    if (use_small && !comm) {
        // Netlib-scale LP: all `count` iterations in one single-workgroup launch, matrices in registers (small.hip)
        launch_small_iterations(small_args(), count, stream);
        return;
    }
    if (!use_graph) {
        for (int i = 0; i < count; ++i) launch_normal_pair(i + 1 < count, nullptr, x_mode_of(i, count));
        return;
    }
    while (count > 0) {
        const int len = std::min(count, kMaxGraphIters);
        HIP_CHECK(hipGraphLaunch(graph_for(len), stream));
        far_A_ready = graph_end_A;
        far_AT_ready = graph_end_AT;
        count -= len;
    }
}

void Solver::run_normal_then_check(int count) {
    // (a fused single-workgroup check + residual launch for Netlib-scale LPs was built and measured in round 4 -- no faster than
    // the eight small launches it replaced, profiles/r04_small_check.txt -- and taken out again in round 5)
    run_normal(count);
    step(true);
}

// ------------------------------------------------------------------------------------------------
// residuals (reference src/main_iterate.cu:229-309).  c.x_bar, y_obj.y_bar, x_bar.z_bar, |x_temp|^2
// and |y_temp|^2 were already reduced by the check-variant epilogues of the step that produced them.
// ------------------------------------------------------------------------------------------------
static double weighted_norm_from(Solver *s, double dot_adx_dy, double dy2, double dx2) {
    const double dot_prod = 2.0 * dot_adx_dy;
    double wn = s->sigma * (s->lambda_max * dy2) + dx2 / s->sigma + dot_prod;
    if (wn < 0) {
        if (s->verbose)
            std::cout << "The estimated maximum eigenvalue is too small! Current value is " << s->lambda_max << "\n";
        s->lambda_max = -(dot_prod + dx2 / s->sigma) / (s->sigma * dy2) * 1.05;
        if (s->verbose) std::cout << "The new estimated maximum eigenvalue is " << s->lambda_max << "\n";
        wn = std::sqrt(-(dot_prod + dx2 / s->sigma) * 0.05);
        s->set_sigma_lambda(s->sigma, s->lambda_max, false);
    } else {
        wn = std::sqrt(wn);
    }
    return wn;
}

void Solver::compute_residuals(int iter, bool compute_gap, Residuals *r, RestartState *rs, bool *ray) {
    residuals_enqueue(iter, compute_gap, ray);
    fetch_wait();
    residuals_consume(iter, compute_gap, r, rs);
}

void Solver::residuals_enqueue(int iter, bool compute_gap, bool *ray) {
    residuals_launch(iter, compute_gap, nullptr);
    if (ray) *ray = ray_test();  // (its scalars ride on the fetch below)
    fetch_enqueue();
}

void Solver::residuals_launch(int iter, bool compute_gap, GroupLaunches *g) {
    invalidate_far();  // the residual SpMVs refill the remainder buffers for x_bar / y_bar
    finish_tiling();
    const int gx = AT.view.grid(), gyy = A.view.grid();
    const int rstride = std::max(stride_x, stride_y);
    gather(gyb.p, true);
    gather(gxb.p, false);
    if (compute_gap) gather(gxt.p, false);
    FinalizeArgs f{};
    if (g) g->resid_d(AT.view, gyb.p, c.p, z_bar.p, col_norm.p, part_x.p);
    else launch_resid_d(AT.view, gyb.p, c.p, z_bar.p, col_norm.p, part_x.p, stream);
    f.item[f.n++] = {part_x.p, gx, S_RD2};
    if (g) g->resid_p(A.view, gxb.p, gxt.p, AL.p, AU.p, row_norm.p, y_temp.p, compute_gap, part_r.p, rstride);
    else launch_resid_p(A.view, gxb.p, gxt.p, AL.p, AU.p, row_norm.p, y_temp.p, compute_gap, part_r.p, rstride, stream);
    f.item[f.n++] = {part_r.p, gyy, S_RP2};
    if (compute_gap) f.item[f.n++] = {part_r.p + rstride, gyy, S_ADX_DY};
    if (iter == 0) {
        if (g) g->lu(n_loc, x_bar, l.p, u.p, col_norm.p, x_temp, part_v.p);  // (resolve_many only: many.cpp)
        else launch_lu(n_loc, x_bar, l.p, u.p, col_norm.p, x_temp, part_v.p, kReduceBlocks, stream);
        f.item[f.n++] = {part_v.p, kReduceBlocks, S_LU2};
    }
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
    allreduce_slots(this, S_CX, 8);
    if (iter == 0) allreduce_slots(this, S_LU2, 1);
}

void Solver::residuals_consume(int iter, bool compute_gap, Residuals *r, RestartState *rs) {
    assemble_residuals(r, {scal_h[S_CX], scal_h[S_YOBJ_Y], scal_h[S_XZ], scal_h[S_RD2], scal_h[S_RP2], scal_h[S_LU2]},
                       {b_scale, c_scale, norm_b_org, norm_c_org, obj_constant}, iter == 0);
    r->kkt = std::max(std::max(r->err_Rd, r->err_Rp), r->rel_gap);  // (batched.hip nests the max() the other way, as the reference)
    if (compute_gap && rs) rs->current_gap = weighted_norm_from(this, scal_h[S_ADX_DY], scal_h[S_DY2], scal_h[S_DX2]);
}

double Solver::weighted_norm_after_restart() {
    gap_launch(nullptr);
    fetch_scalars();
    return weighted_norm_consume();
}

void Solver::gap_launch(GroupLaunches *g) {
    invalidate_far();
    gather(gxt.p, false);
    if (g) g->gap(A.view, gxt.p, y_temp.p, part_r.p);
    else launch_gap(A.view, gxt.p, y_temp.p, part_r.p, stream);
    FinalizeArgs f{};
    f.n = 1;
    f.item[0] = {part_r.p, A.view.grid(), S_ADX_DY};
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
    allreduce_slots(this, S_ADX_DY, 3);  // S_ADX_DY, S_DY2, S_DX2 are adjacent
}

double Solver::weighted_norm_consume() { return weighted_norm_from(this, scal_h[S_ADX_DY], scal_h[S_DY2], scal_h[S_DX2]); }

void Solver::update_sigma_and_restart(RestartState *rs, const Residuals &r) {
    if (rs->flag <= 0) return;
    movement_launch(nullptr);
    fetch_scalars();
    restart_launch(rs, r, nullptr);
}

void Solver::movement_launch(GroupLaunches *g) {
    // movement x_bar - last_x, y_bar - last_y and their norms (update_sigma, main_iterate.cu:367-404)
    if (g) g->movement(n_loc, m_loc, x_bar, last_x.p, x_temp, y_bar, last_y.p, y_temp.p, part_v.p, kReduceBlocks);
    else launch_movement(n_loc, m_loc, x_bar, last_x.p, x_temp, y_bar, last_y.p, y_temp.p, part_v.p, kReduceBlocks, kReduceBlocks, stream);
    FinalizeArgs f{};
    f.n = 2;
    f.item[0] = {part_v.p, kReduceBlocks, S_MOVE_X2};
    f.item[1] = {part_v.p + kReduceBlocks, kReduceBlocks, S_MOVE_Y2};
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
    allreduce_slots(this, S_MOVE_X2, 2);
}

void Solver::restart_launch(RestartState *rs, const Residuals &r, GroupLaunches *g) {
    const double new_sigma = restart_sigma(std::sqrt(scal_h[S_MOVE_X2]), std::sqrt(scal_h[S_MOVE_Y2]), lambda_max, *rs, r);
    // do_restart (main_iterate.cu:312-322) + Halpern reset (:54-66)
    invalidate_far();  // y changes under the remainder buffer of A^T
    if (g) g->restart_copy(n_loc, m_loc, x_bar, x.p, last_x.p, y_bar, y, last_y.p, ctrl.p);
    else launch_restart_copy(n_loc, m_loc, x_bar, x.p, last_x.p, y_bar, y, last_y.p, ctrl.p, stream);
    gather(gy.p, true);
    set_sigma_lambda(new_sigma, lambda_max, true, g);
    rs->inner = 0;
    rs->save_gap = std::numeric_limits<double>::infinity();
}

// ------------------------------------------------------------------------------------------------
// the outer loop (reference src/HPRLP.cu:154-310).  `iter` only ever stops at event iterations
// (periodic check, log line, iteration limit); everything between two events is enqueued at once.
// ------------------------------------------------------------------------------------------------
// (the batched loop stops at periodic checks and the iteration limit only, not at log steps: batched.hip)
static int next_event(int iter, int check_iter, int max_iter) {
    int j = iter + 1;
    while (true) {
        if (j % check_iter == 0 || j % log_step(j) == 0 || j >= max_iter) return j;
        ++j;
    }
}

void Solver::loop_begin(LoopState *ls, HPRLP_results *out, GroupLaunches *g) {
    *ls = LoopState();
    ls->t_loop = time_now();
    // reported `time` includes the power iteration (HPRLP.cu:150); a re-solve ran none and counts its set_data instead
    ls->t_before = time_base >= 0.0 ? time_base : power_time;
    data_since_run = 0.0;
    ls->rs.best_sigma = sigma;
    ls->check_iter = std::max(prm.check_iter, 1);
    ls->max_iter = std::max(prm.max_iter, 0);
    ls->out = out;
    *out = HPRLP_results();
    trace_n = 0;
    cert = Certificate();
    if (detect.on) ray_begin(g);
}

void Solver::loop_enqueue_evaluation(LoopState *ls, GroupLaunches *g, bool fetch) {
    ls->at_limit = ls->iter >= ls->max_iter;
    ls->periodic = (ls->iter % ls->check_iter == 0);
    ls->ray = false;
    residuals_launch(ls->iter, ls->periodic && ls->iter > 0, g);
    if (g) return;  // (the ray test follows the group's kernels: loop_enqueue_ray)
    loop_enqueue_ray(ls);
    if (fetch) fetch_enqueue();
}

bool Solver::loop_enqueue_ray(LoopState *ls, GroupLaunches *g) {
    if (!(detect.on && ls->periodic && ls->iter > 0)) return false;
    ls->ray = ray_test(g);  // (its scalars ride on the copy that follows)
    return true;
}

bool Solver::loop_status(LoopState *ls) {
    const int iter = ls->iter, check_iter = ls->check_iter;
    const bool at_limit = ls->at_limit, periodic = ls->periodic;
    Residuals &r = ls->r;
    RestartState &rs = ls->rs;
    HPRLP_results *out = ls->out;
    std::string &status = ls->status;
    residuals_consume(iter, periodic && iter > 0, &r, &rs);
    const int verdict = ls->ray ? ray_scalars().verdict(detect) : 0;
    const double elapsed = ls->t_before + time_since(ls->t_loop);
    bool timed_out = elapsed > prm.time_limit;  // (strict here, >= in batched.hip, as in the reference)
    if (comm && comm->size > 1) {
        // the residuals are all-reduced, the clocks are not: every rank must take the same TIME_LIMIT decision, or
        // one leaves the loop while its peers enter the next exchange (a collective hang).  Any rank over its limit
        // stops the whole group at this event.
        const double flag = timed_out ? 1.0 : 0.0;
        HIP_CHECK(hipMemcpyAsync(scal.p + S_TMP1, &flag, sizeof(double), hipMemcpyHostToDevice, stream));
        allreduce_slots(this, S_TMP1, 1);
        fetch_scalars();
        timed_out = scal_h[S_TMP1] > 0.0;
    }
    if (r.kkt < prm.stop_tol) status = "OPTIMAL";  // (strict here, <= in batched.hip, as in the reference)
    else if (verdict == 1) status = "PRIMAL_INFEASIBLE";
    else if (verdict == 2) status = "DUAL_INFEASIBLE";
    else if (at_limit) status = "ITER_LIMIT";
    else if (timed_out) status = "TIME_LIMIT";
    if (periodic && !at_limit) check_restart(rs, iter, check_iter, sigma, verbose);
    else rs.flag = 0;
    if (trace && trace_n < trace_cap)
        trace[trace_n++] = TraceRow{iter, rs.flag, r.err_Rp, r.err_Rd, r.primal_obj, r.dual_obj, r.rel_gap, r.kkt,
                                    sigma, rs.current_gap, lambda_max};
    if (verbose) {
        std::cout << std::setw(5) << iter << "    " << std::scientific << std::setprecision(2) << r.err_Rp << "    "
                  << r.err_Rd << "    " << std::setprecision(6) << std::showpos << r.primal_obj << "    "
                  << r.dual_obj << "    " << std::setprecision(2) << std::noshowpos << r.rel_gap << "    " << sigma
                  << "      " << std::fixed << std::setprecision(2) << elapsed << "\n" << std::defaultfloat
                  << std::flush;
    }
    auto mark = [&](bool &first, double thr, int &it_out, double &t_out, const char *label) {
        if (first && r.kkt < thr) {
            it_out = iter;
            t_out = elapsed;
            first = false;
            if (verbose) std::cout << "Residual < " << label << " at iter = " << iter << "\n" << std::flush;
        }
    };
    mark(ls->first4, 1e-4, out->iter4, out->time4, "1e-4");
    mark(ls->first6, 1e-6, out->iter6, out->time6, "1e-6");
    mark(ls->first8, 1e-8, out->iter8, out->time8, "1e-8");
    if (status != "CONTINUE") {
        if (verdict && status != "OPTIMAL") ls->verdict = verdict, ls->verdict_iter = iter;  // (collected by loop_certificate)
        return false;
    }
    ls->restarted = rs.flag > 0;
    return true;
}

void Solver::loop_certificate(LoopState *ls) {
    if (ls->verdict) collect_certificate(ls->verdict, ls->verdict_iter);
}

void Solver::loop_movement(LoopState *, GroupLaunches *g) { movement_launch(g); }

void Solver::loop_restart(LoopState *ls, GroupLaunches *g) {
    restart_launch(&ls->rs, ls->r, g);
    step(true, g);
    gap_launch(g);
}

void Solver::loop_plan(LoopState *ls) {
    const int iter = ls->iter;
    RestartState &rs = ls->rs;
    const int next = next_event(iter, ls->check_iter, ls->max_iter);
    int it = iter;
    if (ls->restarted) {
        rs.last_gap = weighted_norm_consume();
        ++it;
    }
    ls->pending = it < next ? next - 1 - it : -1;
    rs.inner += next - iter;
    ls->iter = next;
}

bool Solver::loop_event(LoopState *ls) {
    loop_enqueue_evaluation(ls);
    fetch_wait();
    if (!loop_status(ls)) {
        loop_certificate(ls);
        return false;
    }
    if (ls->restarted) {
        loop_movement(ls);
        fetch_scalars();
        loop_restart(ls);
        fetch_scalars();
    }
    loop_plan(ls);
    return true;
}

void Solver::loop_advance(LoopState *ls, bool normal_done, GroupLaunches *g) {
    if (ls->pending < 0) return;
    if (normal_done) step(true, g);
    else run_normal_then_check(ls->pending);
}

void Solver::loop_finish(LoopState *ls) {
    HPRLP_results *out = ls->out;
    std::strncpy(out->status, ls->status.c_str(), sizeof(out->status) - 1);
    out->status[sizeof(out->status) - 1] = '\0';
    out->iter = ls->iter;
    out->gap = ls->r.rel_gap;
    out->residuals = ls->r.kkt;
    out->primal_obj = ls->r.primal_obj;
    out->time = ls->t_before + time_since(ls->t_loop);
    if (out->time4 == 0.0) out->time4 = out->time;
    if (out->time6 == 0.0) out->time6 = out->time;
    if (out->time8 == 0.0) out->time8 = out->time;
    if (out->iter4 == 0) out->iter4 = out->iter;
    if (out->iter6 == 0) out->iter6 = out->iter;
    if (out->iter8 == 0) out->iter8 = out->iter;
}

void Solver::solve_loop(HPRLP_results *out) {
    LoopState ls;
    loop_begin(&ls, out);
    if (verbose)
        std::cout << " iter     errRp        errRd         p_obj            d_obj          gap         sigma       time\n"
                  << std::flush;
    while (loop_event(&ls)) loop_advance(&ls);
    if (env_get("HPRLP_TIMING"))
        std::cerr << "[timing] loop: " << time_since(ls.t_loop) << " s, " << ls.iter << " iterations; " << fetches << " scalar fetches: enqueue "
                  << fetch_enqueue_s << " s, wait " << fetch_wait_s << " s" << std::endl;
    loop_finish(&ls);
}

void Solver::collect_solution(HPRLP_results *out) {
    // scratch: sn1 (x), sm1 (y), gsn local slice (z)
    double *zo = gsn.p + col_off;
    solution_launch(sn1.p, sm1.p, zo, nullptr);
    out->x = static_cast<double *>(std::malloc(sizeof(double) * std::max(n_loc, 1)));
    out->y = static_cast<double *>(std::malloc(sizeof(double) * std::max(m_loc, 1)));
    out->z = static_cast<double *>(std::malloc(sizeof(double) * std::max(n_loc, 1)));
    if (!out->x || !out->y || !out->z) throw std::runtime_error("host allocation of the solution failed");
    // (three copies side by side, each driven by its own thread on its own stream, were measured on config 5's 3 x 80 MB: 0.036-0.045 s
    // against 0.017 s for this sequence -- pageable copies serialise inside the runtime)
    HIP_CHECK(hipMemcpyAsync(out->x, sn1.p, sizeof(double) * n_loc, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(out->y, sm1.p, sizeof(double) * m_loc, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(out->z, zo, sizeof(double) * n_loc, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    if (!perm_r.empty()) {  // back to the caller's numbering (reference collect_solution returns the model's order)
        auto unpermute = [](double *v, const std::vector<int> &perm) {
            std::vector<double> tmp(v, v + perm.size());
            for (size_t i = 0; i < perm.size(); ++i) v[perm[i]] = tmp[i];
        };
        unpermute(out->x, perm_c);
        unpermute(out->z, perm_c);
        unpermute(out->y, perm_r);
    }
}

// k_unscale into xo (n_loc), yo (m_loc), zo (n_loc), in the solver's numbering (g: recorded)
void Solver::solution_launch(double *xo, double *yo, double *zo, GroupLaunches *g) {
    if (g) g->unscale(n_loc, m_loc, x_bar, y_bar, z_bar.p, col_norm.p, row_norm.p, b_scale, c_scale, xo, yo, zo);
    else launch_unscale(n_loc, m_loc, x_bar, y_bar, z_bar.p, col_norm.p, row_norm.p, b_scale, c_scale, xo, yo, zo, stream);
}

// ------------------------------------------------------------------------------------------------
// infeasibility detection (DESIGN.md "Infeasibility and unboundedness"): Farkas ratio tests on the difference of the projected
// iterates between two periodic evaluations, in the caller's units.  Single GPU only (abi.cpp refuses sharded solvers).
// ------------------------------------------------------------------------------------------------
void Solver::ray_begin(GroupLaunches *g) {
    if (comm) throw std::runtime_error("infeasibility detection runs on one GPU only (sharded solver)");
    if (!ray_prev_x.p) {
        // (g: fills of +0.0, the bits of the memsets, run by the group's launch ahead of the first evaluation)
        auto zeroed = [&](DBuf<double> &b, int len) {
            if (!g) return b.alloc_zero(static_cast<size_t>(len));
            b.alloc(static_cast<size_t>(len));
            g->fill(b.p, 0.0, len);
        };
        zeroed(ray_prev_x, n_loc);
        zeroed(ray_prev_y, m_loc);
        zeroed(ray_d, n_pad);  // gathered by the ray SpMVs: full padded length
        zeroed(ray_y, m_pad);
    }
    ray_have_prev = false;
}

bool Solver::ray_test(GroupLaunches *rec) {
    finish_tiling();
    const int gx = AT.view.grid(), gyy = A.view.grid();
    const size_t need = static_cast<size_t>(kRayFormAccs) * kReduceBlocks + 2 * static_cast<size_t>(gx) + gyy;
    if (ray_part.n < need) ray_part.alloc(need);
    double *pf = ray_part.p, *pc = pf + static_cast<size_t>(kRayFormAccs) * kReduceBlocks, *pr = pc + 2 * static_cast<size_t>(gx);
    const RayFormArgs a{n_loc, m_loc, x_bar, y_bar, ray_prev_x.p, ray_prev_y.p, ray_d.p, ray_y.p, l.p, u.p, c.p, col_norm.p,
                        AL.p, AU.p, row_norm.p, b_scale, c_scale};
    if (rec) rec->ray_form(a, pf);
    else launch_ray_form(a, pf, kReduceBlocks, stream);
    if (!ray_have_prev) {  // first periodic evaluation: only the stored iterate
        ray_have_prev = true;
        return false;
    }
    FinalizeArgs f{};
    const int form_slots[kRayFormAccs] = {S_RAY_DY, S_RAY_CD, S_RAY_VY, S_RAY_WD, S_RAY_YN, S_RAY_DN};
    for (int k = 0; k < kRayFormAccs; ++k) f.item[f.n++] = {pf + static_cast<size_t>(k) * kReduceBlocks, kReduceBlocks, form_slots[k], k >= 2};
    if (rec) rec->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
    invalidate_far();  // the ray SpMVs refill the remainder buffers
    if (rec) {
        rec->ray_col(AT.view, ray_y.p, l.p, u.p, col_norm.p, b_scale, c_scale, pc);
        rec->ray_row(A.view, ray_d.p, AL.p, AU.p, row_norm.p, b_scale, pr);
    } else {
        launch_ray_col(AT.view, ray_y.p, l.p, u.p, col_norm.p, b_scale, c_scale, pc, stream);
        launch_ray_row(A.view, ray_d.p, AL.p, AU.p, row_norm.p, b_scale, pr, stream);
    }
    FinalizeArgs g{};
    g.item[g.n++] = {pc, gx, S_RAY_DZ, 0};
    g.item[g.n++] = {pc + gx, gx, S_RAY_VZ, 1};
    g.item[g.n++] = {pr, gyy, S_RAY_WQ, 1};
    if (rec) rec->finalize(g, scal.p);
    else launch_finalize(g, scal.p, stream);
    return true;
}

RayScalars Solver::ray_scalars() {
    return RayScalars{scal_h[S_RAY_DY] + scal_h[S_RAY_DZ], std::max(scal_h[S_RAY_VY], scal_h[S_RAY_VZ]), scal_h[S_RAY_CD],
                      std::max(scal_h[S_RAY_WD], scal_h[S_RAY_WQ]), scal_h[S_RAY_YN], scal_h[S_RAY_DN]};
}

void Solver::collect_certificate(int kind, int iter) {
    cert = Certificate();
    std::vector<double> rn(static_cast<size_t>(m_loc)), cn(static_cast<size_t>(n_loc));
    HIP_CHECK(hipMemcpyAsync(rn.data(), row_norm.p, sizeof(double) * m_loc, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(cn.data(), col_norm.p, sizeof(double) * n_loc, hipMemcpyDeviceToHost, stream));
    auto unpermute = [](std::vector<double> &v, const std::vector<int> &perm) {
        if (perm.empty() || v.empty()) return;  // (no ordering, or an array this kind does not use)
        const std::vector<double> tmp(v);
        for (size_t i = 0; i < perm.size(); ++i) v[perm[i]] = tmp[i];
    };
    if (kind == 1) {
        // y and z = -A^T y of the ray; A^T y_s into scratch sn1 by the plain product
        invalidate_far();
        launch_spmv_plain(AT.view, ray_y.p, sn1.p, nullptr, false, nullptr, 0, stream);
        cert.y.resize(static_cast<size_t>(m_loc));
        cert.z.resize(static_cast<size_t>(n_loc));
        HIP_CHECK(hipMemcpyAsync(cert.y.data(), ray_y.p, sizeof(double) * m_loc, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipMemcpyAsync(cert.z.data(), sn1.p, sizeof(double) * n_loc, hipMemcpyDeviceToHost, stream));
    } else {
        cert.d.resize(static_cast<size_t>(n_loc));
        HIP_CHECK(hipMemcpyAsync(cert.d.data(), ray_d.p, sizeof(double) * n_loc, hipMemcpyDeviceToHost, stream));
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    finish_certificate(&cert, kind, iter, ray_scalars(), rn.data(), cn.data(), b_scale, c_scale);
    unpermute(cert.y, perm_r);
    unpermute(cert.z, perm_c);
    unpermute(cert.d, perm_c);
}

void Solver::certificate_launch(int kind, double *rn, double *cn, double *ray, double *aty, GroupLaunches *g) {
    g->copy(cn, col_norm.p, n_loc);
    if (kind == 1) {
        invalidate_far();
        g->copy(rn, row_norm.p, m_loc);
        g->copy(ray, ray_y.p, m_loc);
        g->spmv_plain(AT.view, ray_y.p, aty);  // A^T y_s straight into the block
    } else {
        g->copy(ray, ray_d.p, n_loc);
    }
}

void Solver::certificate_consume(int kind, int iter, const double *rn, const double *cn, const double *ray, const double *aty) {
    cert = Certificate();
    auto unpermute = [](std::vector<double> &v, const std::vector<int> &perm) {  // (collect_certificate's)
        if (perm.empty() || v.empty()) return;
        const std::vector<double> tmp(v);
        for (size_t i = 0; i < perm.size(); ++i) v[perm[i]] = tmp[i];
    };
    if (kind == 1) {
        cert.y.assign(ray, ray + m_loc);
        cert.z.assign(aty, aty + n_loc);
    } else {
        cert.d.assign(ray, ray + n_loc);
    }
    finish_certificate(&cert, kind, iter, ray_scalars(), rn, cn, b_scale, c_scale);
    unpermute(cert.y, perm_r);
    unpermute(cert.z, perm_c);
    unpermute(cert.d, perm_c);
}

// ------------------------------------------------------------------------------------------------
// warm start (DESIGN.md "Warm start"): the caller's point, projected, into the state the first iteration and compute_residuals(0)
// read.  The Halpern anchor is the start itself (last_x, last_y) and the counter stays at 0 (init_iteration_state).
// ------------------------------------------------------------------------------------------------
void Solver::set_start(const double *x0, const double *y0) {
    if (comm) throw std::runtime_error("warm start runs on one GPU only (sharded solver)");
    if (y_exchange_pending) throw std::runtime_error("set_start: an exchange is still pending");
    const auto t0 = time_now();
    finish_tiling();
    invalidate_far();  // y changes under the remainder buffer of A^T, and the SpMVs below refill both buffers
    // the caller's vectors go to the device once, into scratch the kernels below do not write; a locality ordering's permutations
    // travel for this call only (a host gather would be a pass over every entry on the host)
    DBuf<double> dx, dy;
    DBuf<int> dpc, dpr;
    if (x0 && n_loc > 0) {
        dx.alloc(static_cast<size_t>(n_loc));
        HIP_CHECK(hipMemcpyAsync(dx.p, x0, sizeof(double) * n_loc, hipMemcpyHostToDevice, stream));
    }
    if (y0 && m_loc > 0) {
        dy.alloc(static_cast<size_t>(m_loc));
        HIP_CHECK(hipMemcpyAsync(dy.p, y0, sizeof(double) * m_loc, hipMemcpyHostToDevice, stream));
    }
    if (!perm_c.empty() && dx.p) {
        dpc.alloc(perm_c.size());
        HIP_CHECK(hipMemcpyAsync(dpc.p, perm_c.data(), sizeof(int) * perm_c.size(), hipMemcpyHostToDevice, stream));
    }
    if (!perm_r.empty() && dy.p) {
        dpr.alloc(perm_r.size());
        HIP_CHECK(hipMemcpyAsync(dpr.p, perm_r.data(), sizeof(int) * perm_r.size(), hipMemcpyHostToDevice, stream));
    }
    start_apply(dx.p, dy.p, dpc.p, dpr.p);  // (waits for the stream: the uploads' buffers go out of scope here)
    start_time = time_since(t0);
}

// The kernels of a warm start, on device copies of the caller's vectors (caller's numbering; dpc / dpr: device index -> caller's
// index, null without a locality ordering).  Returns after the stream has drained: dx / dy are not read afterwards.
void Solver::start_apply(const double *dx, const double *dy, const int *dpc, const int *dpr) {
    start_launch(dx, dy, dpc, dpr, nullptr);
    HIP_CHECK(hipStreamSynchronize(stream));
}

// start_apply up to its wait (g: recorded; dx / dy must then outlive the group's run)
void Solver::start_launch(const double *dx, const double *dy, const int *dpc, const int *dpr, GroupLaunches *g) {
    const StartInArgs a{n_loc, m_loc, dx, dy, dpc, dpr, l.p, u.p, col_norm.p, AL.p, AU.p, row_norm.p, b_scale, c_scale,
                        x.p, last_x.p, x_hat, x_bar, y, last_y.p, y_bar};
    if (g) g->start_in(a);
    else launch_start_in(a, stream);
    // (one GPU: x_hat, x_bar, y, y_bar are the gathered buffers themselves)
    const int gx = AT.view.grid(), gyy = A.view.grid();
    if (g) g->start_col(AT.view, gyb.p, c.p, l.p, u.p, x_bar, z_bar.p, part_x.p);
    else launch_start_col(AT.view, gyb.p, c.p, l.p, u.p, x_bar, z_bar.p, part_x.p, stream);
    if (g) g->start_row(A.view, gxb.p, AL.p, AU.p, y_bar, y_obj.p, part_r.p);
    else launch_start_row(A.view, gxb.p, AL.p, AU.p, y_bar, y_obj.p, part_r.p, stream);
    FinalizeArgs f{};
    f.item[f.n++] = {part_x.p, gx, S_CX};
    f.item[f.n++] = {part_x.p + gx, gx, S_XZ};
    f.item[f.n++] = {part_r.p, gyy, S_YOBJ_Y};
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
}

// ------------------------------------------------------------------------------------------------
// re-solve (DESIGN.md "Re-solve"): new c / row sides / bounds for the resident model.  Everything that depends on A alone stays
// (scaled matrices, row_norm, col_norm, lambda_max, kernel forms, ordering); the vectors follow the reference's batched rule
// (scale by the cumulative norms, then this data's own b_scale / c_scale and norms).
// ------------------------------------------------------------------------------------------------
void Solver::set_data(const double *c_, const double *obj_constant_, const double *AL_, const double *AU_, const double *l_, const double *u_) {
    if (comm) throw std::runtime_error("new data for a resident model runs on one GPU only (sharded solver)");
    if (!scaled) throw std::runtime_error("set_data: the solver has not been scaled yet (hprlp_solver_scale comes first)");
    const bool bounds = AL_ || AU_ || l_ || u_;
    if (bounds && !(AL_ && AU_ && l_ && u_))
        throw std::runtime_error("set_data: AL, AU, l and u are given together or not at all (b_scale couples them)");
    auto no_nan = [](const double *v, long len, const char *what) {
        for (long i = 0; v && i < len; ++i)
            if (std::isnan(v[i])) throw std::runtime_error(std::string("set_data: ") + what + "[" + std::to_string(i) + "] is NaN");
    };
    no_nan(c_, n, "c"); no_nan(AL_, m, "AL"); no_nan(AU_, m, "AU"); no_nan(l_, n, "l"); no_nan(u_, n, "u");
    if (obj_constant_ && std::isnan(*obj_constant_)) throw std::runtime_error("set_data: obj_constant is NaN");
    data_time[0] = data_time[1] = data_time[2] = 0.0;
    if (obj_constant_) obj_constant = *obj_constant_;
    if (!c_ && !bounds) {
        set_transfer(0, 0, false);
        return;
    }
    const auto t0 = time_now();
    const int mb = bounds ? m_loc : 0, nb = bounds ? n_loc : 0, nc = c_ ? n_loc : 0;
    // staging: [AL | AU | l | u | c]; below the allocator cache's block size the solver keeps it (a hipFree per call would
    // synchronise the device), above it the cache does
    const size_t total = 2 * static_cast<size_t>(mb) + 2 * static_cast<size_t>(nb) + static_cast<size_t>(nc);
    if (data_stage.n < total) data_stage.alloc(total);
    double *dAL = data_stage.p, *dAU = dAL + mb, *dl = dAU + mb, *du = dl + nb, *dc = du + nb;
    const struct { const double *src; double *dst; int len; } parts[5] = {{AL_, dAL, mb}, {AU_, dAU, mb}, {l_, dl, nb}, {u_, du, nb}, {c_, dc, nc}};
    if (total * sizeof(double) < kDeviceCacheMinBytes) {  // one copy instead of five
        data_pack.resize(total);
        for (const auto &q : parts)
            if (q.len > 0) std::memcpy(data_pack.data() + (q.dst - data_stage.p), q.src, sizeof(double) * q.len);
        HIP_CHECK(hipMemcpyAsync(data_stage.p, data_pack.data(), sizeof(double) * total, hipMemcpyHostToDevice, stream));
    } else {
        for (const auto &q : parts)
            if (q.len > 0) HIP_CHECK(hipMemcpyAsync(q.dst, q.src, sizeof(double) * q.len, hipMemcpyHostToDevice, stream));
    }
    data_apply(dAL, dAU, dl, du, c_ ? dc : nullptr, bounds, t0);
    set_transfer(total, 0, false);
}

// set_data from the point where the caller's vectors can be read on the device (the staging block, or the caller's own device
// buffers): k_data_in, k_data_bc, the finalizes, one scalar fetch.  dc null: c not given; bounds false: dAL .. du not read.
void Solver::data_apply(const double *dAL, const double *dAU, const double *dl, const double *du, const double *dc, bool bounds,
                        clock_type::time_point t0) {
    const bool c_ = dc != nullptr;
    perms_to_device();
    if (!data_part.p) data_part.alloc_zero(static_cast<size_t>(4) * kReduceBlocks);
    // The bound codes are written by the second pass into the arrays the iteration kernels (and the captured iteration graphs, by
    // pointer) already read.  The graphs hold nothing else of the data: XHalfArgs / YHalfArgs carry pointers, strides and the
    // hand-off flags, sigma and lambda live in ctrl.  Only a code array that has to be allocated here moves a captured pointer.
    if (!hook_no_bound_codes && bounds) {
        if (row_code.n != static_cast<size_t>(m_loc) || lu_code.n != static_cast<size_t>(n_loc)) {
            for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
            graphs.clear();
            HIP_CHECK(hipStreamSynchronize(stream));
            row_code.alloc(static_cast<size_t>(m_loc));
            lu_code.alloc(static_cast<size_t>(n_loc));
        }
    }
    data_time[0] = time_since(t0);
    const auto t1 = time_now();
    data_first_pass(dAL, dAU, dl, du, dc, bounds, data_part.p, nullptr);
    data_second_pass(bounds, c_, data_part.p, nullptr);
    fetch_scalars();
    data_consume(bounds, c_);
    invalidate_far();
    if (data_stage.cap_bytes >= kDeviceCacheMinBytes) data_stage.release();  // (back to the allocator cache)
    data_time[1] = time_since(t1);
    data_time[2] = time_since(t0);
    data_since_run += data_time[2];
}

// The pieces of data_apply (g: recorded instead of launched; many.cpp: set_data_many).  part: 4 x kReduceBlocks partials -- the
// solver's data_part, or a piece of the group's block (where a partial is stored does not change its value).  The second pass
// reads what the first pass' finalize left in scal: a group records it a stage later.
void Solver::data_first_pass(const double *dAL, const double *dAU, const double *dl, const double *du, const double *dc, bool bounds,
                             double *part, GroupLaunches *g) {
    const bool c_ = dc != nullptr;
    const int mb = bounds ? m_loc : 0, nb = bounds ? n_loc : 0, nc = c_ ? n_loc : 0;
    const DataInArgs in{mb, nc, nb, dAL, dAU, dc, dl, du, perm_c_dev.p, perm_r_dev.p, row_norm.p, col_norm.p,
                        AL.p, AU.p, c.p, l.p, u.p, part, kReduceBlocks};
    if (g) g->data_in(in);
    else launch_data_in(in, stream);
    FinalizeArgs f{};
    if (bounds) {
        f.item[f.n++] = {part, kReduceBlocks, S_DATA_B_ORG};
        f.item[f.n++] = {part + 2 * static_cast<size_t>(kReduceBlocks), kReduceBlocks, S_DATA_B_PRE};
    }
    if (c_) {
        f.item[f.n++] = {part + kReduceBlocks, kReduceBlocks, S_DATA_C_ORG};
        f.item[f.n++] = {part + 3 * static_cast<size_t>(kReduceBlocks), kReduceBlocks, S_DATA_C_PRE};
    }
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
}

void Solver::data_second_pass(bool bounds, bool c_, double *part, GroupLaunches *g) {
    const int mb = bounds ? m_loc : 0, nb = bounds ? n_loc : 0, nc = c_ ? n_loc : 0;
    const bool codes = !hook_no_bound_codes && bounds;
    const DataBcArgs bc{mb, nc, nb, prm.use_bc_scaling ? 1 : 0, scal.p, AL.p, AU.p, c.p, l.p, u.p, codes ? row_code.p : nullptr,
                        codes ? lu_code.p : nullptr, part, kReduceBlocks};
    if (g) g->data_bc(bc);
    else launch_data_bc(bc, stream);
    FinalizeArgs f{};
    if (bounds) f.item[f.n++] = {part, kReduceBlocks, S_DATA_NB};
    if (c_) f.item[f.n++] = {part + kReduceBlocks, kReduceBlocks, S_DATA_NC};
    if (g) g->finalize(f, scal.p);
    else launch_finalize(f, scal.p, stream);
}

// after the scalars have reached scal_h
void Solver::data_consume(bool bounds, bool c_) {
    if (bounds) {
        norm_b_org = 1.0 + std::sqrt(scal_h[S_DATA_B_ORG]);
        b_scale = prm.use_bc_scaling ? 1.0 + std::sqrt(scal_h[S_DATA_B_PRE]) : 1.0;
        norm_b = std::sqrt(scal_h[S_DATA_NB]);
    }
    if (c_) {
        norm_c_org = 1.0 + std::sqrt(scal_h[S_DATA_C_ORG]);
        c_scale = prm.use_bc_scaling ? 1.0 + std::sqrt(scal_h[S_DATA_C_PRE]) : 1.0;
        norm_c = std::sqrt(scal_h[S_DATA_NC]);
    }
}

void Solver::resolve(double sigma_, const double *x0, const double *y0, HPRLP_results *out) {
    if (comm) throw std::runtime_error("re-solve runs on one GPU only (sharded solver)");
    reset_iterates();
    init_iteration_state();
    if (sigma_ > 0.0) set_sigma_lambda(sigma_, lambda_max, true);
    if (x0 || y0) set_start(x0, y0);
    time_base = data_since_run;
    try {
        solve_loop(out);
    } catch (...) {
        time_base = -1.0;
        throw;
    }
    time_base = -1.0;
    collect_solution(out);
    set_transfer((x0 ? n_loc : 0) + static_cast<size_t>(y0 ? m_loc : 0), 2 * static_cast<size_t>(n_loc) + m_loc, false);
}

// ------------------------------------------------------------------------------------------------
// device-resident re-solve (DESIGN.md "Device-resident re-solve"): the entries above with the caller's vectors in device memory.
// The kernels are the host entries'; their sources are the caller's pointers where the host entries pass the staging block.
// ------------------------------------------------------------------------------------------------
void Solver::perms_to_device() {
    if (perm_r.empty() || perm_r_dev.p) return;
    perm_r_dev.alloc(perm_r.size());
    perm_c_dev.alloc(perm_c.size());
    HIP_CHECK(hipMemcpyAsync(perm_r_dev.p, perm_r.data(), sizeof(int) * perm_r.size(), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(perm_c_dev.p, perm_c.data(), sizeof(int) * perm_c.size(), hipMemcpyHostToDevice, stream));
}

void Solver::wait_for_caller(hipStream_t caller) {
    if (!inputs_ready) HIP_CHECK(hipEventCreateWithFlags(&inputs_ready, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(inputs_ready, caller));
    HIP_CHECK(hipStreamWaitEvent(stream, inputs_ready, 0));
}

unsigned long long *Solver::cleared_check_flags() {
    if (!check_flags.p) check_flags.alloc(2);
    HIP_CHECK(hipMemsetAsync(check_flags.p, 0xff, 2 * sizeof(unsigned long long), stream));
    return check_flags.p;
}

void Solver::set_transfer(size_t h2d_words, size_t d2h_words, bool device_entry) {
    transfer[0] = static_cast<long>(h2d_words * sizeof(double));
    transfer[1] = static_cast<long>(d2h_words * sizeof(double));
    transfer[2] = device_entry ? 1 : 0;
    if (device_entry) ++transfer[3];
}

namespace {
// k_data_check's word as the host entries' message: "<who>: <vector>[<index>] <what>"
void throw_if_flagged(unsigned long long word, const char *const names[kDataCheckVecs], const char *who, const char *what) {
    if (word == kDataCheckClean) return;
    const int k = static_cast<int>(word >> kDataCheckShift);
    const unsigned long long i = word & ((1ULL << kDataCheckShift) - 1);
    throw std::runtime_error(std::string(who) + ": " + (k < kDataCheckVecs ? names[k] : "?") + "[" + std::to_string(i) + "] " + what);
}
const char *const kDataNames[kDataCheckVecs] = {"c", "AL", "AU", "l", "u"};
const char *const kStartNames[kDataCheckVecs] = {"x0", "y0", "", "", ""};
}  // namespace

void Solver::set_data_device(const double *dc, const double *obj_constant_, const double *dAL, const double *dAU, const double *dl,
                             const double *du, hipStream_t caller) {
    if (comm) throw std::runtime_error("new data for a resident model runs on one GPU only (sharded solver)");
    if (!scaled) throw std::runtime_error("set_data: the solver has not been scaled yet (hprlp_solver_scale comes first)");
    const bool bounds = dAL || dAU || dl || du;
    if (bounds && !(dAL && dAU && dl && du))
        throw std::runtime_error("set_data: AL, AU, l and u are given together or not at all (b_scale couples them)");
    if (obj_constant_ && std::isnan(*obj_constant_)) throw std::runtime_error("set_data: obj_constant is NaN");
    const auto t0 = time_now();
    // -- no pointer reaches a kernel before all of them have passed
    const char *who = "set_data_device";
    if (dc) check_device_pointer(dc, static_cast<size_t>(n_loc), prm.device_number, "c", who);
    if (bounds) {
        check_device_pointer(dAL, static_cast<size_t>(m_loc), prm.device_number, "AL", who);
        check_device_pointer(dAU, static_cast<size_t>(m_loc), prm.device_number, "AU", who);
        check_device_pointer(dl, static_cast<size_t>(n_loc), prm.device_number, "l", who);
        check_device_pointer(du, static_cast<size_t>(n_loc), prm.device_number, "u", who);
    }
    if (dc || bounds) {
        const double t_ptr = time_since(t0);
        wait_for_caller(caller);
        const double t_ev = time_since(t0);
        unsigned long long *flag = cleared_check_flags();
        const DataCheckArgs chk{{dc, dAL, dAU, dl, du}, {n_loc, m_loc, m_loc, n_loc, n_loc}, 0};
        launch_data_check(chk, flag, stream);
        unsigned long long first_bad = kDataCheckClean;
        HIP_CHECK(hipMemcpyAsync(&first_bad, flag, sizeof(first_bad), hipMemcpyDeviceToHost, stream));
        const double t_enq = time_since(t0);
        HIP_CHECK(hipStreamSynchronize(stream));
        if (env_get("HPRLP_TIMING"))
            std::cerr << "[timing] set_data_device: pointer checks " << t_ptr << " s, event " << t_ev - t_ptr << " s, check enqueued "
                      << t_enq - t_ev << " s, wait " << time_since(t0) - t_enq << " s" << std::endl;
        throw_if_flagged(first_bad, kDataNames, "set_data", "is NaN");
    }
    // -- from here on the call goes through
    data_time[0] = data_time[1] = data_time[2] = 0.0;
    if (obj_constant_) obj_constant = *obj_constant_;
    if (dc || bounds) {
        data_apply(dAL, dAU, dl, du, dc, bounds, t0);  // (ends with the scalar fetch: the stream has drained)
    }
    set_transfer(0, 0, true);
}

void Solver::resolve_device(double sigma_, const double *dx0, const double *dy0, hipStream_t caller, double *dx, double *dy, double *dz,
                            HPRLP_results *out) {
    if (comm) throw std::runtime_error("re-solve runs on one GPU only (sharded solver)");
    const char *who = "resolve_device";
    if (dx0) check_device_pointer(dx0, static_cast<size_t>(n_loc), prm.device_number, "x0", who);
    if (dy0) check_device_pointer(dy0, static_cast<size_t>(m_loc), prm.device_number, "y0", who);
    if (dx) check_device_pointer(dx, static_cast<size_t>(n_loc), prm.device_number, "x", who);
    if (dy) check_device_pointer(dy, static_cast<size_t>(m_loc), prm.device_number, "y", who);
    if (dz) check_device_pointer(dz, static_cast<size_t>(n_loc), prm.device_number, "z", who);
    wait_for_caller(caller);  // (the outputs too: what the caller's stream still does with them comes first)
    if (dx0 || dy0) {
        unsigned long long *flag = cleared_check_flags();
        const DataCheckArgs chk{{dx0, dy0, nullptr, nullptr, nullptr}, {n_loc, m_loc, 0, 0, 0}, 1};
        launch_data_check(chk, flag, stream);
        unsigned long long first_bad = kDataCheckClean;
        HIP_CHECK(hipMemcpyAsync(&first_bad, flag, sizeof(first_bad), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        throw_if_flagged(first_bad, kStartNames, "warm start", "is not finite");
    }
    reset_iterates();
    init_iteration_state();
    if (sigma_ > 0.0) set_sigma_lambda(sigma_, lambda_max, true);
    if (dx0 || dy0) {  // set_start with the caller's buffers where it uploads copies; consumed here, so dx / dy may be the same buffers
        if (y_exchange_pending) throw std::runtime_error("set_start: an exchange is still pending");
        const auto t0 = time_now();
        finish_tiling();
        invalidate_far();
        perms_to_device();
        start_apply(dx0, dy0, dx0 ? perm_c_dev.p : nullptr, dy0 ? perm_r_dev.p : nullptr);
        start_time = time_since(t0);
    }
    time_base = data_since_run;
    try {
        solve_loop(out);
    } catch (...) {
        time_base = -1.0;
        throw;
    }
    time_base = -1.0;
    out->x = out->y = out->z = nullptr;
    if (dx || dy || dz) {
        perms_to_device();
        launch_unscale_out(n_loc, m_loc, x_bar, y_bar, z_bar.p, col_norm.p, row_norm.p, b_scale, c_scale, perm_c_dev.p, perm_r_dev.p, dx, dy,
                           dz, stream);
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    set_transfer(0, 0, true);
}

}  // namespace hprlp
