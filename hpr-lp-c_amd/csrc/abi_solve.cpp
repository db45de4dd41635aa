// abi_solve.cpp -- extern "C" boundary, the one-call solves: the reference's entry points (include/HPRLP.h: HPRLP_main_solve,
// solve), hprlp_solve_detect / _warm with the single certificate, the warm-up, hprlp_last_error / hprlp_backend and the phases,
// and the presolve as separate steps.  The helpers of abi_common.h that start here are defined here.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <mutex>

#include "abi_common.h"
#include "env.h"
#include "presolve.h"
#include "version.h"

using namespace hprlp;

HPRLP_results hprlp::make_error_result(const char *status) {
    HPRLP_results r;
    std::memset(r.status, 0, sizeof(r.status));
    std::strncpy(r.status, status, sizeof(r.status) - 1);
    r.residuals = r.primal_obj = r.gap = 0.0;
    return r;
}

static void print_banner_and_parameters(const HPRLP_parameters *p) {
    std::cout << "\n==================================================================\n"
              << "                 HPR-LP Solver  (MI355X / gfx950 HIP build)       \n"
              << "     Halpern Peaceman-Rachford Linear Programming Solver          \n"
              << "  Version: " << HPRLP_VERSION_STRING << "   backend: " << HPRLP_BACKEND_STRING << "\n"
              << "==================================================================\n\n";
    std::cout << "Solver Parameters:\n"
              << "  Device:              GPU " << p->device_number << "\n"
              << "  Max Iterations:      " << p->max_iter << "\n"
              << "  Stopping Tolerance:  " << std::scientific << std::setprecision(1) << p->stop_tol << "\n"
              << std::defaultfloat << "  Time Limit:          " << std::fixed << std::setprecision(1) << p->time_limit
              << " seconds\n" << std::defaultfloat << "  Check Interval:      " << p->check_iter << " iterations\n"
              << "  PSLP Presolve:       " << (p->use_presolve ? "Enabled" : "Disabled") << "\n"
              << "  Scaling:  CR=" << p->use_CR_scaling << " Ruiz=" << p->use_Ruiz_scaling
              << " Pock-Chambolle=" << p->use_Pock_Chambolle_scaling << " b/c=" << p->use_bc_scaling << "\n\n";
}

extern "C" const char *hprlp_last_error(void) { return last_error_cstr(); }
extern "C" const char *hprlp_backend(void) { return HPRLP_BACKEND_STRING; }

// ---- warm-up -------------------------------------------------------------------------------------------------------
// The first solve of a process pays for the HIP runtime's start-up, the device context, the first stream and the library's code
// objects (loaded as their first kernels are launched): 0.10 s on a Netlib-scale LP whose solve takes 0.04 s
// (profiles/r04_cold_start.txt).  None of it depends on the LP.  hprlp_warmup() does it on request -- a serving process calls
// it once at start-up, the first solve() then costs what the later ones do plus the first stream (0.03 s).  Measured and NOT
// done: starting it implicitly from the model constructors on a background thread -- a context first touched by another
// thread cost the solving thread MORE set-up time (0.18 instead of 0.09 s), and loading all six code objects up front is
// 0.05 s of which a small solve needs 0.01.
namespace hprlp {
void warm_kernels_tu();
void warm_small_tu();
void warm_batched_tu();
void warm_transpose_tu();
void warm_tiled_build_tu();
void warm_reorder_tu();
}  // namespace hprlp

static double g_warm_seconds[4] = {0, 0, 0, 0};

extern "C" int hprlp_warmup(int device) {
    const auto t0 = time_now();
    int count = 0;
    if (hipInit(0) != hipSuccess || hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        set_last_error("hprlp_warmup: no usable GPU");
        return -1;
    }
    if (device < 0 || device >= count) {
        set_last_error("hprlp_warmup: device " + std::to_string(device) + " is outside [0, " + std::to_string(count) + ")");
        return -1;
    }
    const auto t1 = time_now();
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess || hipStreamCreate(&s) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("hprlp_warmup: the device context could not be created");
        return -1;
    }
    (void)hipStreamDestroy(s);
    const auto t2 = time_now();
    // one attribute query per translation unit loads that unit's code object (deferred loading: otherwise at its first launch)
    int rc = 0;
    try {
        warm_kernels_tu();
        warm_small_tu();
        warm_batched_tu();
        warm_transpose_tu();
        warm_tiled_build_tu();
        warm_reorder_tu();
    } catch (const std::exception &e) {
        set_last_error(std::string("hprlp_warmup: a code object did not load: ") + e.what());
        rc = -2;
    } catch (...) {
        set_last_error("hprlp_warmup: a code object did not load");
        rc = -2;
    }
    (void)hipGetLastError();
    const auto t3 = time_now();
    g_warm_seconds[0] = std::chrono::duration<double>(t1 - t0).count();
    g_warm_seconds[1] = std::chrono::duration<double>(t2 - t1).count();
    g_warm_seconds[2] = std::chrono::duration<double>(t3 - t2).count();
    g_warm_seconds[3] = std::chrono::duration<double>(t3 - t0).count();
    if (env_get("HPRLP_TIMING"))
        std::cerr << "[timing] warm-up: runtime start-up " << g_warm_seconds[0] << " s, device context + first stream " << g_warm_seconds[1]
                  << " s, code objects " << g_warm_seconds[2] << " s" << std::endl;
    return rc;
}

// The drop-in path (round 5).  A caller that comes through the reference's unchanged bindings cannot call hprlp_warmup(): the
// model constructors do the process-wide part on the CALLING thread, once -- runtime start-up, device 0's context and first
// stream, and the two code objects every solve launches from (kernels.hip, small.hip; the others load with their first kernel:
// a Netlib-scale solve never pays for the tiled builders).  Quiet: a host without a GPU builds models as before (solves fail
// loudly later).  The cost moves from the first solve() to the first create_model_* (profiles/r05_cold_start.txt); the
// background-thread form of round 4 stays rejected (a context first touched by another thread cost the solver more).
namespace hprlp {
void warm_for_first_solve() {
    if (env_on("HPRLP_NO_WARM_MODEL")) return;  // (a process that forks after building its models: INTEGRATION.md)
    static std::once_flag once;
    std::call_once(once, []() {
        const auto t0 = time_now();
        int count = 0;
        if (hipInit(0) != hipSuccess || hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
            (void)hipGetLastError();
            return;
        }
        hipStream_t s = nullptr;
        if (hipSetDevice(0) == hipSuccess && hipFree(nullptr) == hipSuccess && hipStreamCreate(&s) == hipSuccess) (void)hipStreamDestroy(s);
        try {
            warm_kernels_tu();
            warm_small_tu();
        } catch (...) {
        }
        (void)hipGetLastError();
        if (env_get("HPRLP_TIMING")) std::cerr << "[timing] warm-up at model creation: " << time_since(t0) << " s" << std::endl;
    });
}
}  // namespace hprlp

extern "C" int hprlp_warmup_seconds(double out[4]) { return read_counts(g_warm_seconds, out); }

// phases of the calling thread's last HPRLP_main_solve (hprlp_last_solve_phases): device set-up (upload, transpose, tiled
// copies, ordering), scaling, power iteration, loop, solution's way back, teardown of the device state, whole call
static thread_local double g_phases[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_solve_phases(double out[8]) { return read_counts(g_phases, out); }

static void free_xyz(HPRLP_results &r) {
    std::free(r.x); std::free(r.y); std::free(r.z);
    r.x = r.y = r.z = nullptr;
}

// reference src/HPRLP.cu:116-311.  det (may be null: off, as in the reference) switches the infeasibility detection on; a verdict's
// certificate goes to *cert.  x0 / y0 (both null: the reference's cold start from zero): warm start (Solver::set_start).
static HPRLP_results main_solve(const LP_info_cpu *model, const HPRLP_parameters *param, const Detection *det, Certificate *cert,
                                const double *x0 = nullptr, const double *y0 = nullptr) {
    if (!model || !param) {
        std::cerr << "[error] Null model or parameter pointer" << std::endl;
        return make_error_result("ERROR");
    }
    const auto t_call = time_now();
    try {
        print_banner_and_parameters(param);
        HPRLP_results out;
        auto t_down = time_now();
        {
        Solver s;
        s.setup(model, param);
        std::cout << "Setup (copy and allocation) time = " << std::fixed << std::setprecision(2) << s.setup_time
                  << " seconds" << std::endl;
        s.scale();
        std::cout << "Scaling time = " << std::fixed << std::setprecision(2) << s.scaling_time << " seconds" << std::endl;
        s.lambda_max = s.power_iteration(5000, 1e-4, nullptr) * 1.01;  // src/HPRLP.cu:81-97
        if (s.power_iters >= 5000)
            std::cout << "Power iteration did not converge within the specified tolerance.\n";
        std::cout << "ESTIMATING MAXIMUM EIGENVALUE time = " << std::fixed << std::setprecision(2) << s.power_time
                  << " seconds" << std::endl << std::defaultfloat;
        s.init_iteration_state();
        if (det) s.detect = *det;
        if (x0 || y0) s.set_start(x0, y0);
        const auto t_loop = time_now();
        s.solve_loop(&out);
        const double loop_s = time_since(t_loop);
        if (cert) *cert = std::move(s.cert);
        const auto t_col = time_now();
        s.collect_solution(&out);
        g_phases[0] = s.setup_time; g_phases[1] = s.scaling_time; g_phases[2] = s.power_time; g_phases[3] = loop_s;
        g_phases[4] = time_since(t_col);
        g_phases[7] = (x0 || y0) ? s.start_time : 0.0;
        t_down = time_now();
        }  // (the solver's device state goes here: part of the call's wall time)
        g_phases[5] = time_since(t_down);
        g_phases[6] = time_since(t_call);
        std::cout << "\n=== Solution Summary ===\n"
                  << "Status: " << out.status << "\nIterations: " << out.iter << "\nTime: " << out.time
                  << " seconds\nPrimal Objective: " << std::scientific << std::setprecision(12) << out.primal_obj
                  << "\nResidual: " << out.residuals << "\n\n" << std::defaultfloat;
        return out;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        std::cerr << "[error] HPRLP_main_solve failed: " << e.what() << std::endl;
        return make_error_result("ERROR");
    }
}

extern "C" HPRLP_results HPRLP_main_solve(const LP_info_cpu *model, const HPRLP_parameters *param) {
    return main_solve(model, param, nullptr, nullptr);
}

// ---- solve(): reference src/HPRLP.cu:493-524 -------------------------------------------------------------------------------
// With use_presolve (the default) the model is first reduced on the host (presolve.h -- our own in-process presolver where the
// reference forks a PSLP worker, src/pslp_integration.cpp:628-713), the reduced model goes through HPRLP_main_solve and the
// result is mapped back to the original dimensions and checked against the original model (src/pslp_integration.cpp:715-787).
// If the presolver declines, the original model is solved.  solve_impl below is the sequence; its steps come first.

// NULL if the CSR arrays of `model` are consistent, else what is wrong with them.
static const char *invalid_model_reason(const LP_info_cpu *model) {
    const sparseMatrix *A = model->A;
    if (model->m <= 0 || model->n <= 0) return "model dimensions must be positive";
    if (!A || !A->rowPtr || !A->colIndex || !A->value) return "model matrix arrays missing";
    if (!model->AL || !model->AU || !model->l || !model->u || !model->c) return "model vectors missing";
    if (A->row != model->m || A->col != model->n) return "model matrix dimensions inconsistent";
    if (A->rowPtr[0] != 0) return "row pointer array does not start at 0";
    for (int i = 0; i < model->m; ++i)
        if (A->rowPtr[i + 1] < A->rowPtr[i]) return "row pointer array is not monotone";
    if (A->rowPtr[model->m] != A->numElements) return "row pointer array does not end at numElements";
    for (int k = 0; k < A->numElements; ++k)
        if (A->colIndex[k] < 0 || A->colIndex[k] >= model->n) return "column index out of range";
    return nullptr;
}

static bool is_verdict(const HPRLP_results &r) {
    return std::strcmp(r.status, "PRIMAL_INFEASIBLE") == 0 || std::strcmp(r.status, "DUAL_INFEASIBLE") == 0;
}

// x, y, z of the model's dimensions on the malloc heap (hprlp_free_results frees them); false, and nothing allocated, without memory
static bool alloc_xyz(const LP_info_cpu *model, double **x, double **y, double **z) {
    *x = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
    *y = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->m, 1)));
    *z = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
    if (*x && *y && *z) return true;
    std::free(*x); std::free(*y); std::free(*z);
    *x = *y = *z = nullptr;
    return false;
}

// The fallback: the model as given, within what is left of the caller's time and iteration limits after `spent` seconds
// (presolve and the reduced solve, wall clock since entry) and `it_first` iterations; so do the reported times and counts
static HPRLP_results solve_original_rest(const LP_info_cpu *model, const HPRLP_parameters *p, const Detection *det, Certificate *cert,
                                         const double *x0, const double *y0, double spent, int it_first) {
    HPRLP_parameters p2 = *p;
    p2.time_limit = std::max(p->time_limit - spent, 0.0);
    p2.max_iter = std::max(p->max_iter - it_first, 0);
    if (cert) *cert = Certificate();  // (only the original model's verdicts count)
    HPRLP_results r2 = main_solve(model, &p2, det, cert, x0, y0);
    if (std::strcmp(r2.status, "ERROR") != 0) {
        // iter4/6/8 of a tolerance the second solve never reached are back-filled with its final count
        // (reference src/HPRLP.cu:248-253): offset like `iter`, so they stay "<= iter"
        r2.time += spent; r2.time4 += spent; r2.time6 += spent; r2.time8 += spent;
        r2.iter += it_first; r2.iter4 += it_first; r2.iter6 += it_first; r2.iter8 += it_first;
        if (cert && cert->kind) cert->iter += it_first;  // (detection: the verdict's iteration counts the same way)
    }
    return r2;
}

// The presolver indexes its work arrays by the model's column indices and trusts rowPtr: a hand-built LP_info_cpu
// (create_model_from_arrays validates, a caller-filled struct does not) must be refused before any host array is touched --
// without presolve DeviceMatrix::upload refuses the same models.  True: refused, with the message left and printed.
static bool refuse_invalid_model(const LP_info_cpu *model) {
    const char *why = invalid_model_reason(model);
    if (!why) return false;
    set_last_error(why);
    std::cerr << "[error] invalid model: " << why << std::endl;
    return true;
}

// true: pre holds a reduced model.  A presolve that fails is a presolve that declined.
static bool run_presolve(Presolve &pre, const LP_info_cpu *model) {
    try {
        std::cout << "Doing presolve..." << std::endl;
        const bool reduced = pre.run(model);
        std::cout << "Presolve time: " << pre.stats().seconds << " seconds" << std::endl;
        return reduced;
    } catch (const std::exception &e) {
        std::cerr << "[warn] presolve failed (" << e.what() << "); solving original model" << std::endl;
        return false;
    }
}

// The reductions removed every row and column: the undo sequence alone produces a primal-dual optimum.  True: *r is the
// call's result ("OPTIMAL" with that point; "ERROR" without memory).  False: the point failed the original model's KKT check.
static bool presolve_only_result(const Presolve &pre, const LP_info_cpu *model, const HPRLP_parameters *p, HPRLP_results *r) {
    *r = make_error_result("ERROR");
    if (!alloc_xyz(model, &r->x, &r->y, &r->z)) return true;
    pre.postsolve(nullptr, nullptr, nullptr, r->x, r->y, r->z);
    const OriginalKkt k = original_kkt(model, r->x, r->y, r->z);
    r->primal_obj = k.primal_obj;
    r->gap = k.gap;
    r->residuals = std::max(k.primal_feas, std::max(k.dual_feas, k.gap));
    r->time = r->time4 = r->time6 = r->time8 = pre.stats().seconds;
    r->iter = r->iter4 = r->iter6 = r->iter8 = 0;
    if (r->residuals <= p->stop_tol) {
        std::strncpy(r->status, "OPTIMAL", sizeof(r->status) - 1);  // (over "ERROR" in a zeroed field)
        return true;
    }
    free_xyz(*r);
    return false;
}

// The stopping test is relative to 1 + |b| and 1 + |c| of the model it runs on, and slack substitution moves cost between
// columns (|c| of the reduced model can be several times the original's): the same absolute residuals would then pass on the
// reduced model and fail the original-model check.  The reduced solve gets the tolerance that corresponds to stop_tol on the
// ORIGINAL norms.
static HPRLP_parameters reduced_parameters(const LP_info_cpu *model, const LP_info_cpu *reduced, const HPRLP_parameters *p) {
    auto norm_bc = [](const LP_info_cpu *mod, double *nb, double *nc) {
        double sb = 0.0, sc = 0.0;
        for (int i = 0; i < mod->m; ++i) {
            const double a = std::isinf(mod->AL[i]) ? 0.0 : std::abs(mod->AL[i]), b = std::isinf(mod->AU[i]) ? 0.0 : std::abs(mod->AU[i]);
            const double v = std::max(a, b);
            sb += v * v;
        }
        for (int j = 0; j < mod->n; ++j) sc += mod->c[j] * mod->c[j];
        *nb = std::sqrt(sb);
        *nc = std::sqrt(sc);
    };
    double nb0, nc0, nb1, nc1;
    norm_bc(model, &nb0, &nc0);
    norm_bc(reduced, &nb1, &nc1);
    HPRLP_parameters pr = *p;
    const double shrink = std::min(1.0, std::min((1.0 + nb0) / (1.0 + nb1), (1.0 + nc0) / (1.0 + nc1)));
    if (shrink < 1.0) {
        pr.stop_tol = p->stop_tol * shrink;
        std::cout << "Reduced-model tolerance " << pr.stop_tol << " (original norms |b| " << nb0 << ", |c| " << nc0 << "; reduced "
                  << nb1 << ", " << nc1 << ")" << std::endl;
    }
    return pr;
}

// The caller's start carried into the reduced model (a missing half: zeros); xr / yr stay empty for a cold start
static void forward_start(const Presolve &pre, const LP_info_cpu *model, const double *x0, const double *y0, std::vector<double> *xr,
                          std::vector<double> *yr) {
    if (!x0 && !y0) return;
    std::vector<double> xf(x0 ? x0 : nullptr, x0 ? x0 + model->n : nullptr), yf(y0 ? y0 : nullptr, y0 ? y0 + model->m : nullptr);
    xf.resize(static_cast<size_t>(model->n), 0.0);
    yf.resize(static_cast<size_t>(model->m), 0.0);
    xr->resize(static_cast<size_t>(pre.reduced()->n));
    yr->resize(static_cast<size_t>(pre.reduced()->m));
    pre.forward(xf.data(), yf.data(), xr->data(), yr->data());
}

// r's solution of the reduced model becomes one of the model as given; false (r's arrays freed) without memory
static bool postsolve_result(const Presolve &pre, const LP_info_cpu *model, HPRLP_results *r) {
    double *x, *y, *z;
    if (!alloc_xyz(model, &x, &y, &z)) {
        free_xyz(*r);
        return false;
    }
    pre.postsolve(r->x, r->y, r->z, x, y, z);
    free_xyz(*r);
    r->x = x; r->y = y; r->z = z;
    return true;
}

// The postsolved optimum against the ORIGINAL model's KKT conditions, reported.  True when it misses them by orders of
// magnitude: a reduction went wrong on this input, and the model as given has to be solved rather than a wrong answer handed back.
static bool postsolved_point_is_far_off(const LP_info_cpu *model, const HPRLP_results &r, const HPRLP_parameters *p) {
    const OriginalKkt k = original_kkt(model, r.x, r.y, r.z);
    const double err = std::max(k.primal_feas, std::max(k.dual_feas, k.gap));
    if (err <= p->stop_tol) {
        std::cout << "Postsolve original KKT check passed" << std::endl;
        return false;
    }
    std::cout << "Warning: postsolve original KKT check failed (the primal solution and objective are reliable)\n"
              << "  Primal Residual: " << k.primal_feas << "  Dual Residual: " << k.dual_feas
              << "  Relative Gap: " << k.gap << "  (tolerance " << p->stop_tol << ")" << std::endl;
    return err > 100.0 * p->stop_tol && err > 1e-3;
}

// det / cert: infeasibility detection (hprlp_solve_detect), null for solve().  x0 / y0: warm start of the model as given (hprlp_solve_warm),
// both null for a cold start; the reduced solve starts from their image under the presolve's forward map.
static HPRLP_results solve_impl(const LP_info_cpu *model, const HPRLP_parameters *param, const Detection *det, Certificate *cert,
                                const double *x0 = nullptr, const double *y0 = nullptr) {
    if (!model) {
        std::cerr << "[error] Null model pointer" << std::endl;
        return make_error_result("ERROR");
    }
    HPRLP_parameters dflt;
    const HPRLP_parameters *p = param ? param : &dflt;
    if (!p->use_presolve) return main_solve(model, p, det, cert, x0, y0);
    const auto t_entry = time_now();  // (the fallbacks below charge everything since here against the caller's time limit)
    if (refuse_invalid_model(model)) return make_error_result("ERROR");

    Presolve pre;
    const bool reduced = run_presolve(pre, model);
    if (!reduced && pre.solved()) {
        std::cout << "Presolve solved the model (no rows or columns left)" << std::endl;
        HPRLP_results r;
        if (presolve_only_result(pre, model, p, &r)) return r;
        // (cannot happen with exact arithmetic; with rounding trouble fall back to the iteration)
        std::cout << "Postsolve-only solution failed the KKT check; solving original model" << std::endl;
        return main_solve(model, p, det, cert, x0, y0);
    }
    if (!reduced) {
        std::cout << "Presolve left the model unchanged; solving original model" << std::endl;
        return main_solve(model, p, det, cert, x0, y0);
    }
    const Presolve::Stats &st = pre.stats();
    std::cout << "Presolve reduced problem: (" << model->m << ", " << model->n << ") -> (" << pre.reduced()->m << ", "
              << pre.reduced()->n << ")  [fixed cols " << st.fixed_cols << ", empty cols " << st.empty_cols
              << ", dual-fixed cols " << st.dual_fixed_cols << ", slack cols " << st.slack_cols << ", parallel rows " << st.parallel_rows << ", parallel cols " << st.parallel_cols << ", forcing rows " << st.forcing_rows << ", singleton rows " << st.singleton_rows << ", empty rows " << st.empty_rows << ", redundant rows "
              << st.redundant_rows << ", doubleton rows " << st.doubleton_rows << ", tightened bounds " << st.tightened_bounds << "; " << st.rounds
              << " rounds]" << std::endl;
    const HPRLP_parameters pr = reduced_parameters(model, pre.reduced(), p);
    std::vector<double> xr, yr;
    forward_start(pre, model, x0, y0, &xr, &yr);
    HPRLP_results r = main_solve(pre.reduced(), &pr, det, cert, xr.empty() ? nullptr : xr.data(), yr.empty() ? nullptr : yr.data());
    if (det && is_verdict(r)) {
        // a certificate of the reduced model is no certificate of the caller's: solve the model as given, with detection
        free_xyz(r);
        const double spent = time_since(t_entry);
        std::cout << "Reduced model ended " << r.status << " at iteration " << r.iter << "; solving the original model for its certificate"
                  << std::endl;
        return solve_original_rest(model, p, det, cert, x0, y0, spent, r.iter);
    }
    if (det && cert) *cert = Certificate();  // (only the original model's verdicts count)
    if (!(r.x && r.y && r.z)) return r;
    if (!postsolve_result(pre, model, &r)) {
        std::cerr << "[error] out of memory in postsolve" << std::endl;
        return make_error_result("ERROR");
    }
    if (std::strcmp(r.status, "OPTIMAL") != 0) {
        std::cout << "Skipping postsolve original KKT check since the reduced solution is not optimal" << std::endl;
        return r;
    }
    if (!postsolved_point_is_far_off(model, r, p)) return r;
    std::cout << "Postsolved solution is far from the original model's KKT conditions; solving the original model" << std::endl;
    free_xyz(r);
    const double spent = time_since(t_entry);
    const HPRLP_results r2 = solve_original_rest(model, p, det, cert, x0, y0, spent, r.iter);
    std::cout << "Fallback solve: reported time and iterations include presolve and the reduced solve (" << spent
              << " s, " << r.iter << " iterations)" << std::endl;
    return r2;
}

extern "C" HPRLP_results solve(const LP_info_cpu *model, const HPRLP_parameters *param) {
    return solve_impl(model, param, nullptr, nullptr);
}

// ---- detection, warm start and the single certificate ---------------------------------------------------------------------
void hprlp::clear_certificate(hprlp_certificate *c, int m, int n) {
    std::memset(c, 0, sizeof(*c));
    c->m = m;
    c->n = n;
}

// Certificate -> hprlp_certificate (malloc'd arrays)
bool hprlp::export_certificate(const Certificate &k, hprlp_certificate *c, int m, int n) {
    clear_certificate(c, m, n);
    auto dup = [](const std::vector<double> &v, double **out) {
        if (v.empty()) return true;
        *out = static_cast<double *>(std::malloc(sizeof(double) * v.size()));
        if (!*out) return false;
        std::memcpy(*out, v.data(), sizeof(double) * v.size());
        return true;
    };
    if (!dup(k.y, &c->y) || !dup(k.z, &c->z) || !dup(k.d, &c->d)) {
        hprlp_free_certificate(c);
        clear_certificate(c, m, n);
        return false;
    }
    c->kind = k.kind;
    c->iter = k.iter;
    c->objective = k.objective;
    c->violation = k.violation;
    return true;
}

bool hprlp::detection_from(const hprlp_detection *d, Detection *out) {
    if (!d) return false;
    if (!(d->eps_primal_infeasible >= 0.0) || !(d->eps_dual_infeasible >= 0.0))
        throw std::runtime_error("infeasibility detection: eps_primal_infeasible and eps_dual_infeasible must be >= 0");
    out->on = true;
    out->eps_primal = d->eps_primal_infeasible;
    out->eps_dual = d->eps_dual_infeasible;
    return true;
}

void hprlp::check_start(const double *v, long len, const char *what) {
    if (!v) return;
    for (long i = 0; i < len; ++i)
        if (!std::isfinite(v[i]))
            throw std::runtime_error(std::string("warm start: ") + what + "[" + std::to_string(i) + "] is not finite");
}

// hprlp_solve_detect and hprlp_solve_warm (`who`, for the error messages).  No detection and no start: exactly solve().  The
// certificate is cleared on entry and filled only when detection ran; a start is checked before any device work.
static HPRLP_results solve_entry(const LP_info_cpu *model, const HPRLP_parameters *param, const double *x0, const double *y0,
                                 const hprlp_detection *det, hprlp_certificate *cert, const char *who) {
    const int m = model ? model->m : 0, n = model ? model->n : 0;
    const bool warm = x0 || y0;
    if (cert) clear_certificate(cert, m, n);
    if (!det && !warm) return solve(model, param);
    return guarded(make_error_result("ERROR"), [&] {
        try {
            if (warm) {
                if (!model) throw std::runtime_error("null model");
                check_start(x0, n, "x0");
                check_start(y0, m, "y0");
            }
            Detection d;
            const bool with_det = detection_from(det, &d);
            Certificate k;
            HPRLP_results r = solve_impl(model, param, with_det ? &d : nullptr, with_det ? &k : nullptr, x0, y0);
            if (std::strcmp(r.status, "ERROR") == 0 && !*last_error_cstr()) set_last_error(std::string(who) + ": the solve failed");
            if (cert && with_det && !export_certificate(k, cert, m, n)) {
                free_xyz(r);
                throw std::runtime_error("host allocation of the certificate failed");
            }
            return r;
        } catch (const std::exception &e) {
            std::cerr << "[error] " << who << " failed: " << e.what() << std::endl;
            throw;
        }
    });
}

extern "C" HPRLP_results hprlp_solve_detect(const LP_info_cpu *model, const HPRLP_parameters *param, const hprlp_detection *det,
                                            hprlp_certificate *cert) {
    return solve_entry(model, param, nullptr, nullptr, det, cert, "hprlp_solve_detect");
}

extern "C" HPRLP_results hprlp_solve_warm(const LP_info_cpu *model, const HPRLP_parameters *param, const double *x0, const double *y0,
                                          const hprlp_detection *det, hprlp_certificate *cert) {
    if (!x0 && !y0) return hprlp_solve_detect(model, param, det, cert);
    return solve_entry(model, param, x0, y0, det, cert, "hprlp_solve_warm");
}

extern "C" void hprlp_free_certificate(hprlp_certificate *cert) {
    if (!cert) return;
    std::free(cert->y);
    std::free(cert->z);
    std::free(cert->d);
    cert->y = cert->z = cert->d = nullptr;
    cert->kind = 0;
}

// ---- presolve as separate steps (host only; used by the CPU tests and by callers that want the maps) ----------------------
struct hprlp_presolve {
    Presolve p;
};
extern "C" hprlp_presolve *hprlp_presolve_run(const LP_info_cpu *model) {
    hprlp_presolve *h = nullptr;
    hprlp_presolve *made = guarded(static_cast<hprlp_presolve *>(nullptr), [&]() -> hprlp_presolve * {
        h = new hprlp_presolve();
        if (h->p.run(model)) return h;
        set_last_error("presolve left the model unchanged");
        return nullptr;
    });
    if (!made) delete h;
    return made;
}
extern "C" const LP_info_cpu *hprlp_presolve_reduced(const hprlp_presolve *h) { return h ? h->p.reduced() : nullptr; }
extern "C" int hprlp_presolve_stats(const hprlp_presolve *h, int out[16]) {
    if (!h || !out) return -1;
    const Presolve::Stats &s = h->p.stats();
    out[0] = h->p.reduced()->m; out[1] = h->p.reduced()->n; out[2] = s.fixed_cols; out[3] = s.empty_cols;
    out[4] = s.singleton_rows; out[5] = s.empty_rows; out[6] = s.redundant_rows; out[7] = s.passes;
    out[8] = s.dual_fixed_cols; out[9] = s.slack_cols; out[10] = s.parallel_rows; out[11] = s.parallel_cols;
    out[12] = s.forcing_rows; out[13] = s.doubleton_rows; out[14] = s.tightened_bounds; out[15] = s.rounds;
    return 0;
}
extern "C" int hprlp_presolve_postsolve(const hprlp_presolve *h, const double *xr, const double *yr, const double *zr,
                                        double *x, double *y, double *z) {
    if (!h || !xr || !yr || !zr || !x || !y || !z) return -1;
    h->p.postsolve(xr, yr, zr, x, y, z);
    return 0;
}
extern "C" int hprlp_presolve_forward(const hprlp_presolve *h, const double *x, const double *y, double *xr, double *yr) {
    if (!h || !x || !y || !xr || !yr) return -1;
    h->p.forward(x, y, xr, yr);
    return 0;
}
extern "C" void hprlp_presolve_free(hprlp_presolve *h) { delete h; }
extern "C" int hprlp_original_kkt(const LP_info_cpu *model, const double *x, const double *y, const double *z,
                                  double out[5]) {
    if (!model || !model->A || !x || !y || !z || !out) return -1;
    const OriginalKkt k = original_kkt(model, x, y, z);
    out[0] = k.primal_feas; out[1] = k.dual_feas; out[2] = k.gap; out[3] = k.primal_obj; out[4] = k.dual_obj;
    return 0;
}
