// abi_tools.cpp -- extern "C" boundary, the entries that take no solver handle: the locality ordering whole and step by step,
// the tiling share and the row-block plan of a pattern, the value maps, the form selection and the tiled structure restated
// on the host, the table of environment switches, the stream schedule and the shared-memory transport's selftest.
#include <algorithm>
#include <memory>

#include "abi_common.h"
#include "env.h"
#include "reorder.h"
#include "stream_schedule.h"
#include "values.h"

using namespace hprlp;

// Locality ordering of a CSR pattern (reorder.cpp), host only: out = {accepted (0/1), tiled share of the entries before,
// after, clusters, components, seconds}; the permutations (new -> old) are written only when accepted.
extern "C" int hprlp_locality_ordering(int m, int n, const int *rowptr, const int *col, int *row_new2old, int *col_new2old, double out[6]) {
    return guarded(-1, [&] {
        if (m <= 0 || n <= 0 || !rowptr || !col || !row_new2old || !col_new2old) throw std::runtime_error("bad arguments");
        std::vector<int> pr, pc;
        ReorderStats st;
        const bool ok = locality_ordering(m, n, rowptr, col, &pr, &pc, &st);
        if (ok) {
            std::copy(pr.begin(), pr.end(), row_new2old);
            std::copy(pc.begin(), pc.end(), col_new2old);
        }
        if (out) {
            out[0] = ok ? 1.0 : 0.0; out[1] = st.fraction_before; out[2] = st.fraction_after;
            out[3] = st.clusters; out[4] = st.components; out[5] = st.seconds;
        }
        return 0;
    });
}

// ---- the ordering step by step (test infrastructure; tests/test_reorderref.py, tests/test_gpu_reorder_steps.py)
static void check_pattern(int m, int n, const int *rp, const int *ci) {
    if (m <= 0 || n <= 0 || !rp || !ci) throw std::runtime_error("bad arguments");
    if (rp[0] != 0) throw std::runtime_error("rowptr[0] != 0");
    for (int i = 0; i < m; ++i)
        if (rp[i + 1] < rp[i]) throw std::runtime_error("rowptr decreases");
    if (rp[m] <= 0) throw std::runtime_error("no entries");
    for (int k = 0; k < rp[m]; ++k)
        if (ci[k] < 0 || ci[k] >= n) throw std::runtime_error("column index out of range");
}

static void check_permutation(int len, const int *p, const char *what) {
    std::vector<char> seen(static_cast<size_t>(len), 0);
    for (int i = 0; i < len; ++i) {
        if (p[i] < 0 || p[i] >= len || seen[p[i]]) throw std::runtime_error(std::string(what) + " is not a permutation");
        seen[p[i]] = 1;
    }
}

extern "C" int hprlp_reorder_steps(int m, int n, const int *rowptr, const int *col, int on_device, int sweeps, int *lab_r, int *lab_c,
                                   double *pos0_r, double *pos0_c, double *pos_r, double *pos_c, int *row_new2old, int *col_new2old,
                                   double stats[5]) {
    return guarded(-1, [&] {
        check_pattern(m, n, rowptr, col);
        if (sweeps < 0) throw std::runtime_error("negative sweep count");
        const long nnz = rowptr[m];
        const size_t M = static_cast<size_t>(m), N = static_cast<size_t>(n);
        std::vector<int> trp, tci, lr(M), lc(N), hr, hc;
        transpose_pattern(m, n, rowptr, col, trp, tci);
        ReorderStats st;
        std::vector<double> p0r, p0c, pr, pc;
        if (on_device) {
            hipStream_t s = nullptr;
            DBuf<int> drp(M + 1), dci(static_cast<size_t>(nnz)), dtrp(N + 1), dtci(static_cast<size_t>(nnz)), d_r(M), d_c(N);
            drp.upload(rowptr, M + 1);
            dci.upload(col, static_cast<size_t>(nnz));
            dtrp.upload(trp.data(), N + 1);
            dtci.upload(tci.data(), static_cast<size_t>(nnz));
            DBuf<double> dpr(M), dpc(N);
            st.fraction_before = device_tiling_dense_fraction(m, n, nnz, drp.p, dci.p, nullptr, nullptr, s);
            device_cluster_positions(m, n, nnz, drp.p, dci.p, dtrp.p, dtci.p, dpr.p, dpc.p, &st, s, lr.data(), lc.data());
            p0r.resize(M); p0c.resize(N); pr.resize(M); pc.resize(N); hr.resize(M); hc.resize(N);
            dpr.download(p0r.data(), M);
            dpc.download(p0c.data(), N);
            device_refine_order(m, n, drp.p, dci.p, dtrp.p, dtci.p, dpr.p, dpc.p, sweeps, d_r.p, d_c.p, s);
            dpr.download(pr.data(), M);
            dpc.download(pc.data(), N);
            d_r.download(hr.data(), M);
            d_c.download(hc.data(), N);
            check_permutation(m, hr.data(), "the device's row_new2old");  // (before it indexes anything on the device)
            check_permutation(n, hc.data(), "the device's col_new2old");
            st.fraction_after = device_tiling_dense_fraction(m, n, nnz, drp.p, dci.p, d_r.p, d_c.p, s);
        } else {
            st.fraction_before = tiling_dense_fraction(m, n, rowptr, col, nullptr, nullptr);
            cluster_positions(m, n, rowptr, col, trp.data(), tci.data(), &p0r, &p0c, &st, &lr, &lc);
            pr = p0r;
            pc = p0c;
            refine_order(m, n, rowptr, col, trp.data(), tci.data(), pr, pc, sweeps, &hr, &hc);
            std::vector<int> c_old2new(N);
            for (int j = 0; j < n; ++j) c_old2new[hc[j]] = j;
            st.fraction_after = tiling_dense_fraction(m, n, rowptr, col, hr.data(), c_old2new.data());
        }
        if (lab_r) std::copy(lr.begin(), lr.end(), lab_r);
        if (lab_c) std::copy(lc.begin(), lc.end(), lab_c);
        if (pos0_r) std::copy(p0r.begin(), p0r.end(), pos0_r);
        if (pos0_c) std::copy(p0c.begin(), p0c.end(), pos0_c);
        if (pos_r) std::copy(pr.begin(), pr.end(), pos_r);
        if (pos_c) std::copy(pc.begin(), pc.end(), pos_c);
        if (row_new2old) std::copy(hr.begin(), hr.end(), row_new2old);
        if (col_new2old) std::copy(hc.begin(), hc.end(), col_new2old);
        if (stats) {
            stats[0] = st.clusters; stats[1] = st.components; stats[2] = st.bfs_levels;
            stats[3] = st.fraction_before; stats[4] = st.fraction_after;
        }
        return 0;
    });
}

extern "C" int hprlp_permute_csr_device(int m, int n, const int *rowptr, const int *col, const double *val, const int *row_new2old,
                                        const int *col_new2old, int *rp_out, int *ci_out, double *val_out) {
    return guarded(-1, [&] {
        check_pattern(m, n, rowptr, col);
        if (!val || !row_new2old || !col_new2old || !rp_out || !ci_out || !val_out) throw std::runtime_error("bad arguments");
        check_permutation(m, row_new2old, "row_new2old");
        check_permutation(n, col_new2old, "col_new2old");
        const size_t M = static_cast<size_t>(m), N = static_cast<size_t>(n), Z = static_cast<size_t>(rowptr[m]);
        DBuf<int> drp(M + 1), dci(Z), d_r(M), d_c(N), orp(M + 1), oci(Z);
        DBuf<double> dv(Z), ov(Z);
        drp.upload(rowptr, M + 1);
        dci.upload(col, Z);
        dv.upload(val, Z);
        d_r.upload(row_new2old, M);
        d_c.upload(col_new2old, N);
        device_permute_csr(m, n, static_cast<long>(Z), drp.p, dci.p, dv.p, d_r.p, d_c.p, orp.p, oci.p, ov.p, nullptr);
        orp.download(rp_out, M + 1);
        oci.download(ci_out, Z);
        ov.download(val_out, Z);
        return 0;
    });
}

extern "C" int hprlp_tiling_share(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                                  int on_device, double *share) {
    return guarded(-1, [&] {
        check_pattern(m, n, rowptr, col);
        if (!share || (row_new2old == nullptr) != (col_new2old == nullptr)) throw std::runtime_error("bad arguments");
        if (row_new2old) {
            check_permutation(m, row_new2old, "row_new2old");
            check_permutation(n, col_new2old, "col_new2old");
        }
        const size_t M = static_cast<size_t>(m), N = static_cast<size_t>(n), Z = static_cast<size_t>(rowptr[m]);
        if (on_device) {
            DBuf<int> drp(M + 1), dci(Z), d_r, d_c;
            drp.upload(rowptr, M + 1);
            dci.upload(col, Z);
            if (row_new2old) {
                d_r.alloc(M);
                d_c.alloc(N);
                d_r.upload(row_new2old, M);
                d_c.upload(col_new2old, N);
            }
            *share = device_tiling_dense_fraction(m, n, static_cast<long>(Z), drp.p, dci.p, d_r.p, d_c.p, nullptr);
        } else if (row_new2old) {
            std::vector<int> c_old2new(N);
            for (int j = 0; j < n; ++j) c_old2new[col_new2old[j]] = j;
            *share = tiling_dense_fraction(m, n, rowptr, col, row_new2old, c_old2new.data());
        } else {
            *share = tiling_dense_fraction(m, n, rowptr, col, nullptr, nullptr);
        }
        return 0;
    });
}

// Host only: the stream kernel's row blocks of a CSR pattern (split rows, chunks by column eighths), built and checked as a
// solver's set-up does.  out = {blocks, split rows, chunk slots, rows cut by column eighths, longest chunk, entries covered}.
extern "C" int hprlp_row_block_plan(int m, int n, const int *rowptr, const int *col, int with_cuts, long out[6]) {
    return guarded(-1, [&] {
        if (m <= 0 || n <= 0 || !rowptr || !col || !out) throw std::runtime_error("bad arguments");
        row_block_plan_host(m, n, rowptr, col, with_cuts != 0, out);
        return 0;
    });
}

// Host only: the rule of the value maps restated (values_host.cpp); row_new2old / col_new2old null: no ordering
extern "C" int hprlp_value_maps_host(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                                     int *mapA, int *mapAT) {
    return guarded(-1, [&] {
        value_maps_host(m, n, rowptr, col, row_new2old, col_new2old, mapA, mapAT);
        return 0;
    });
}

// Host only: the staged decisions of the kernel-form selection (form_select.h) for a facts record
extern "C" int hprlp_form_select(const hprlp_form_facts *facts, const hprlp_form_hooks *hooks, hprlp_form_decision *out) {
    return guarded(-1, [&] {
        if (!facts || !out) throw std::runtime_error("bad arguments");
        const char *missing = "";
        if (!form_select(*facts, hooks ? *hooks : FormHooks(), out, &missing))
            throw std::runtime_error(std::string("the rules ask for a fact that the record marks as not measured: ") + missing);
        return 0;
    });
}

// Host only: the column-tiled structure of a CSR pattern (host builder, tiled.cpp) with super-blocks of R rows and tiles of T
// columns, verified entry by entry (every entry once, codes name their entries, one chunk per accumulator inside a step, layers).
// out = {tile entries incl. padding, remainder entries, steps, padding, most consecutive steps of one tile, staged share x 1e6}.
extern "C" int hprlp_tiled_host_check(int m, int n, const int *rowptr, const int *col, int R, int T, double min_dense, long out[6]) {
    return guarded(-1, [&] {
        if (m <= 0 || n <= 0 || !rowptr || !col || !out) throw std::runtime_error("bad arguments");
        tiled_host_check(m, n, rowptr, col, R, T, min_dense, out);
        return 0;
    });
}

// The table of environment switches (env.h) as text, one per line: "<name>\t<integrator|hook>\t<what>"; returns the length.
extern "C" int hprlp_env_switches(char *buf, int cap) {
    int count = 0;
    const EnvEntry *t = env_table(&count);
    std::string d;
    for (int i = 0; i < count; ++i) d += std::string(t[i].name) + "\t" + (t[i].kind == EnvKind::Integrator ? "integrator" : "hook") + "\t" + t[i].what + "\n";
    if (buf && cap > 0) std::snprintf(buf, static_cast<size_t>(cap), "%s", d.c_str());
    return static_cast<int>(d.size());
}

extern "C" int hprlp_stream_schedule_host(int count, int width, const int *events, int *slot, int *event_in, int *event_out) {
    return guarded(-1, [&] { return stream_schedule(count, width, events, slot, event_in, event_out); });
}
extern "C" int hprlp_stream_schedule_parents_host(int count, int width, const int *events, const int *parent, int *slot, int *event_in,
                                                  int *event_out) {
    return guarded(-1, [&] { return stream_schedule_parents(count, width, events, parent, slot, event_in, event_out); });
}

// The shared-memory transport's protocol on HOST buffers (no GPU, no HIP call): rank `rank` of `size` attaches to the group the
// id names and runs `rounds` rounds of all-gather, scalar all-reduce and a neighbour exchange whose payloads every receiver
// checks.  hang_rank >= 0: that rank leaves before round `rounds / 2` without a word (the others must end with an error once
// HPRLP_DIST_TIMEOUT_S has passed, not wait for ever).  Returns 0, or -1 + hprlp_last_error().
extern "C" int hprlp_shm_transport_selftest(const void *unique_id, int id_bytes, int rank, int size, int rounds, int hang_rank) {
    return guarded(-1, [&] {
        const int chunk = 1000 + 7;
        std::unique_ptr<Comm> c(make_shm_comm(rank, size, unique_id, static_cast<size_t>(id_bytes), sizeof(double) * chunk * static_cast<size_t>(size), -1));
        std::vector<double> g(static_cast<size_t>(chunk) * size), sc(3);
        std::vector<std::vector<double>> snd(size), rcv(size);
        for (int it = 0; it < rounds; ++it) {
            if (rank == hang_rank && it == rounds / 2) return 0;
            std::fill(g.begin(), g.end(), -1.0);
            for (int j = 0; j < chunk; ++j) g[static_cast<size_t>(rank) * chunk + j] = 1e6 * it + 1e3 * rank + j;
            c->allgather_inplace(g.data(), chunk, nullptr);
            for (int p = 0; p < size; ++p)
                for (int j = 0; j < chunk; ++j)
                    if (g[static_cast<size_t>(p) * chunk + j] != 1e6 * it + 1e3 * p + j) throw std::runtime_error("all-gather delivered a wrong entry");
            sc[0] = rank + 1.0; sc[1] = it; sc[2] = 0.1 * (rank + 1);
            c->allreduce_sum(sc.data(), 3, nullptr);
            double want2 = 0.0;
            for (int p = 0; p < size; ++p) want2 += 0.1 * (p + 1);
            if (sc[0] != size * (size + 1) / 2.0 || sc[1] != static_cast<double>(it) * size || sc[2] != want2) throw std::runtime_error("all-reduce gave a wrong sum");
            // rank a sends (a + 2 b + it) % 5 + (b > a) doubles to rank b: ragged, some empty
            std::vector<P2P> ops;
            for (int p = 0; p < size; ++p) {
                if (p == rank) continue;
                const size_t ns = static_cast<size_t>((rank + 2 * p + it) % 5 + (p > rank)), nr = static_cast<size_t>((p + 2 * rank + it) % 5 + (rank > p));
                snd[p].assign(ns, 0.0);
                for (size_t j = 0; j < ns; ++j) snd[p][j] = 100.0 * rank + p + 0.001 * static_cast<double>(j) + it;
                rcv[p].assign(nr, -7.0);
                if (ns || nr) ops.push_back(P2P{p, snd[p].data(), ns * sizeof(double), rcv[p].data(), nr * sizeof(double)});
            }
            c->exchange(ops.data(), static_cast<int>(ops.size()), nullptr);
            for (int p = 0; p < size; ++p)
                for (size_t j = 0; p != rank && j < rcv[p].size(); ++j)
                    if (rcv[p][j] != 100.0 * p + rank + 0.001 * static_cast<double>(j) + it) throw std::runtime_error("exchange delivered a wrong entry");
        }
        return 0;
    });
}
