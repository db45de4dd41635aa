// solver_values.cpp -- Solver::set_matrix_values and the value maps (DESIGN.md "Matrix values"): new matrix values for the resident
// pattern.  Everything that depends on the pattern alone stays (index arrays, ordering, kernel forms, tiled layouts, row-block
// lists, small-path tables, captured graphs); the values, the five vectors and everything scale() derives from them are
// those of a fresh solver on the changed model.
#include <cmath>

#include "reorder.h"
#include "solver.h"
#include "values.h"

namespace hprlp {

// The maps are built with the code that built the matrices: positions 0 .. nnz-1 travel as doubles (exact below 2^53) through
// device_permute_csr / device_transpose / csr_transpose_host in the values' place and come back as ints.
void Solver::build_value_maps() {
    if (have_maps) return;
    if (comm) throw std::runtime_error("value maps: one GPU only (sharded solver)");
    const long nnz = A.view.nnz;
    DBuf<int> bad;
    bad.alloc_zero(1);
    DBuf<int> new_A, new_AT;
    new_AT.alloc(static_cast<size_t>(std::max<long>(nnz, 1)));
    if (nnz > 0) {
        DBuf<double> pos(static_cast<size_t>(nnz)), out(static_cast<size_t>(nnz));
        launch_positions(pos.p, nnz, stream);
        if (!perm_r.empty()) {
            if (!src_rowptr.p || !src_col.p) throw std::runtime_error("value maps: the caller's pattern is no longer on the device");
            if (!perm_r_dev.p) {
                perm_r_dev.alloc(perm_r.size());
                perm_c_dev.alloc(perm_c.size());
                HIP_CHECK(hipMemcpyAsync(perm_r_dev.p, perm_r.data(), sizeof(int) * perm_r.size(), hipMemcpyHostToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(perm_c_dev.p, perm_c.data(), sizeof(int) * perm_c.size(), hipMemcpyHostToDevice, stream));
            }
            DBuf<int> rp(static_cast<size_t>(m) + 1), ci(static_cast<size_t>(nnz)), trp(static_cast<size_t>(n) + 1);
            // P A Q as try_reorder() formed it: out[e] = the caller's position of entry e of A
            device_permute_csr(m, n, nnz, src_rowptr.p, src_col.p, pos.p, perm_r_dev.p, perm_c_dev.p, rp.p, ci.p, out.p, stream);
            new_A.alloc(static_cast<size_t>(nnz));
            launch_positions_to_int(out.p, nnz, new_A.p, bad.p, stream);
            // ... and its transpose as setup() formed it, on the resident index arrays
            device_transpose(m, n, nnz, A.rowptr.p, A.col.p, out.p, trp.p, ci.p, pos.p, stream);
            launch_positions_to_int(pos.p, nnz, new_AT.p, bad.p, stream);
        } else if (device_transposed) {
            DBuf<int> trp(static_cast<size_t>(n) + 1), tci(static_cast<size_t>(nnz));
            device_transpose(m, n, nnz, A.rowptr.p, A.col.p, pos.p, trp.p, tci.p, out.p, stream);
            launch_positions_to_int(out.p, nnz, new_AT.p, bad.p, stream);
        } else {  // few nonzeros: the host transpose, on the index arrays as the device holds them
            std::vector<int> rp(static_cast<size_t>(m) + 1), ci(static_cast<size_t>(nnz)), trp, tci;
            A.rowptr.download(rp.data(), rp.size());
            A.col.download(ci.data(), ci.size());
            std::vector<double> p(static_cast<size_t>(nnz)), tv;
            for (long k = 0; k < nnz; ++k) p[k] = static_cast<double>(k);
            csr_transpose_host(m, n, nnz, rp.data(), ci.data(), p.data(), trp, tci, tv);
            out.upload(tv.data(), tv.size());
            launch_positions_to_int(out.p, nnz, new_AT.p, bad.p, stream);
        }
        HIP_CHECK(hipStreamSynchronize(stream));  // the temporaries are released on return
    }
    int b = 0;
    bad.download(&b, 1);
    if (b) throw std::runtime_error("value maps: a position outside the matrix (internal error)");
    map_A = std::move(new_A);
    map_AT = std::move(new_AT);
    src_rowptr.release();
    src_col.release();
    have_maps = true;
}

void Solver::set_matrix_values(const double *val, long nnz, const double *c_, const double *obj_constant_, const double *AL_,
                               const double *AU_, const double *l_, const double *u_) {
    if (comm) throw std::runtime_error("set_matrix_values: new matrix values for a resident model run on one GPU only (sharded solver)");
    if (!scaled) throw std::runtime_error("set_matrix_values: the solver has not been scaled yet (hprlp_solver_scale comes first)");
    if (!val || !c_ || !AL_ || !AU_ || !l_ || !u_)
        throw std::runtime_error("set_matrix_values: val, c, AL, AU, l and u are all required (every scaled vector depends on the values)");
    if (nnz != static_cast<long>(A.view.nnz))
        throw std::runtime_error("set_matrix_values: nnz is " + std::to_string(nnz) + ", the model has " + std::to_string(A.view.nnz) +
                                 " entries (the pattern cannot change)");
    auto no_nan = [](const double *v, long len, const char *what) {
        for (long i = 0; i < len; ++i)
            if (std::isnan(v[i])) throw std::runtime_error(std::string("set_matrix_values: ") + what + "[" + std::to_string(i) + "] is NaN");
    };
    no_nan(c_, n, "c"); no_nan(AL_, m, "AL"); no_nan(AU_, m, "AU"); no_nan(l_, n, "l"); no_nan(u_, n, "u");
    if (obj_constant_ && std::isnan(*obj_constant_)) throw std::runtime_error("set_matrix_values: obj_constant is NaN");
    const auto t0 = time_now();
    double times[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (!have_maps) {
        build_value_maps();
        times[0] = time_since(t0);
    }
    // staging: [val | AL | AU | l | u | c]; below the allocator cache's block size the solver keeps it, above it the cache does
    const auto t_up = time_now();
    const size_t nz = static_cast<size_t>(nnz), total = nz + 2 * static_cast<size_t>(m) + 3 * static_cast<size_t>(n);
    if (matrix_stage.n < total) matrix_stage.alloc(total);
    struct Unstage {  // (also on the way out of a refusal)
        DBuf<double> &b;
        ~Unstage() {
            if (b.cap_bytes >= kDeviceCacheMinBytes) b.release();
        }
    } unstage{matrix_stage};
    double *dval = matrix_stage.p, *dAL = dval + nz, *dAU = dAL + m, *dl = dAU + m, *du = dl + n, *dc = du + n;
    const struct { const double *src; double *dst; size_t len; } parts[6] = {{val, dval, nz}, {AL_, dAL, static_cast<size_t>(m)},
        {AU_, dAU, static_cast<size_t>(m)}, {l_, dl, static_cast<size_t>(n)}, {u_, du, static_cast<size_t>(n)}, {c_, dc, static_cast<size_t>(n)}};
    if (total * sizeof(double) < kDeviceCacheMinBytes) {  // one copy instead of six
        data_pack.resize(total);
        for (const auto &q : parts)
            if (q.len > 0) std::memcpy(data_pack.data() + (q.dst - matrix_stage.p), q.src, sizeof(double) * q.len);
        HIP_CHECK(hipMemcpyAsync(matrix_stage.p, data_pack.data(), sizeof(double) * total, hipMemcpyHostToDevice, stream));
    } else {
        for (const auto &q : parts)
            if (q.len > 0) HIP_CHECK(hipMemcpyAsync(q.dst, q.src, sizeof(double) * q.len, hipMemcpyHostToDevice, stream));
    }
    if (!perm_r.empty() && !perm_r_dev.p) {
        perm_r_dev.alloc(perm_r.size());
        perm_c_dev.alloc(perm_c.size());
        HIP_CHECK(hipMemcpyAsync(perm_r_dev.p, perm_r.data(), sizeof(int) * perm_r.size(), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(perm_c_dev.p, perm_c.data(), sizeof(int) * perm_c.size(), hipMemcpyHostToDevice, stream));
    }
    if (!values_flag.p) values_flag.alloc(1);
    HIP_CHECK(hipMemsetAsync(values_flag.p, 0xff, sizeof(unsigned long long), stream));
    // nothing the solver reads has been written yet: the staged values are checked where they are
    launch_values_check(dval, nnz, values_flag.p, stream);
    unsigned long long first_bad = kValuesAllFinite;
    HIP_CHECK(hipMemcpyAsync(&first_bad, values_flag.p, sizeof(first_bad), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    times[1] = time_since(t_up);
    if (first_bad != kValuesAllFinite)
        throw std::runtime_error("set_matrix_values: val[" + std::to_string(first_bad) + "] is not finite");
    // -- from here on the call goes through
    values_apply(dval, nnz, dAL, dAU, dl, du, dc, obj_constant_, t0, times);
    set_transfer(total, 0, false);
}

// set_matrix_values from the point where the values and the vectors have been checked where they lie on the device (the staging
// block, or the caller's own buffers): the scatter through the value maps, the gather of the vectors, iterates to zero, scale().
void Solver::values_apply(const double *dval, long nnz, const double *dAL, const double *dAU, const double *dl, const double *du,
                          const double *dc, const double *obj_constant_, clock_type::time_point t0, double times[5]) {
    const auto t_k = time_now();
    launch_values_in(nnz, dval, map_A.p, map_AT.p, A.val.p, AT.val.p, stream);
    const VectorsInArgs vin{m_loc, n_loc, dAL, dAU, dl, du, dc, perm_r_dev.p, perm_c_dev.p, AL.p, AU.p, l.p, u.p, c.p};
    launch_vectors_in(vin, stream);
    if (obj_constant_) obj_constant = *obj_constant_;
    // Iterates, work vectors, device scalars and ctrl as a fresh solver has them (zero), so that scale() and the power iteration
    // start from the same bits.  The captured graphs stay: they hold pointers, strides and hand-off flags, sigma and lambda live
    // in ctrl, and no kernel form, grid or table depends on a value.
    reset_iterates();
    times[2] = time_since(t_k);
    scale();  // (invalidate_far, the tiled / remainder copies refreshed from the new CSR values, bound codes, norms, scales)
    times[3] = scaling_time;
    times[4] = time_since(t0);
    for (int i = 0; i < 5; ++i) matrix_time[i] = times[i];
    ++matrix_calls;
    data_since_run += times[4];
}

// The device entry (DESIGN.md "Device-resident re-solve"): the caller's device buffers take the staging block's place.
void Solver::set_matrix_values_device(const double *dval, long nnz, const double *dc, const double *obj_constant_, const double *dAL,
                                      const double *dAU, const double *dl, const double *du, hipStream_t caller) {
    if (comm) throw std::runtime_error("set_matrix_values: new matrix values for a resident model run on one GPU only (sharded solver)");
    if (!scaled) throw std::runtime_error("set_matrix_values: the solver has not been scaled yet (hprlp_solver_scale comes first)");
    if (!dval || !dc || !dAL || !dAU || !dl || !du)
        throw std::runtime_error("set_matrix_values: val, c, AL, AU, l and u are all required (every scaled vector depends on the values)");
    if (nnz != static_cast<long>(A.view.nnz))
        throw std::runtime_error("set_matrix_values: nnz is " + std::to_string(nnz) + ", the model has " + std::to_string(A.view.nnz) +
                                 " entries (the pattern cannot change)");
    if (obj_constant_ && std::isnan(*obj_constant_)) throw std::runtime_error("set_matrix_values: obj_constant is NaN");
    // -- no pointer reaches a kernel before all of them have passed
    const auto t_ptr = time_now();
    const char *who = "set_matrix_values_device";
    check_device_pointer(dval, static_cast<size_t>(nnz), prm.device_number, "val", who);
    check_device_pointer(dc, static_cast<size_t>(n), prm.device_number, "c", who);
    check_device_pointer(dAL, static_cast<size_t>(m), prm.device_number, "AL", who);
    check_device_pointer(dAU, static_cast<size_t>(m), prm.device_number, "AU", who);
    check_device_pointer(dl, static_cast<size_t>(n), prm.device_number, "l", who);
    check_device_pointer(du, static_cast<size_t>(n), prm.device_number, "u", who);
    const double ptr_seconds = time_since(t_ptr);
    const auto t0 = time_now();
    double times[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (!have_maps) {
        build_value_maps();
        times[0] = time_since(t0);
    }
    const auto t_up = time_now();
    wait_for_caller(caller);
    perms_to_device();
    // nothing the solver reads has been written yet: values and vectors are checked where they are, both words in one fetch
    unsigned long long *flags = cleared_check_flags();
    const DataCheckArgs chk{{dc, dAL, dAU, dl, du}, {n, m, m, n, n}, 0};
    launch_data_check(chk, flags, stream);
    launch_values_check(dval, nnz, flags + 1, stream);
    unsigned long long first_bad[2] = {kDataCheckClean, kValuesAllFinite};
    HIP_CHECK(hipMemcpyAsync(first_bad, flags, sizeof(first_bad), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    times[1] = ptr_seconds + time_since(t_up);
    if (first_bad[0] != kDataCheckClean) {
        const char *const names[kDataCheckVecs] = {"c", "AL", "AU", "l", "u"};
        const int k = static_cast<int>(first_bad[0] >> kDataCheckShift);
        throw std::runtime_error(std::string("set_matrix_values: ") + (k < kDataCheckVecs ? names[k] : "?") + "[" +
                                 std::to_string(first_bad[0] & ((1ULL << kDataCheckShift) - 1)) + "] is NaN");
    }
    if (first_bad[1] != kValuesAllFinite)
        throw std::runtime_error("set_matrix_values: val[" + std::to_string(first_bad[1]) + "] is not finite");
    // -- from here on the call goes through
    values_apply(dval, nnz, dAL, dAU, dl, du, dc, obj_constant_, t0, times);
    HIP_CHECK(hipStreamSynchronize(stream));  // (the caller's buffers are not read after the return)
    set_transfer(0, 0, true);
}

}  // namespace hprlp
