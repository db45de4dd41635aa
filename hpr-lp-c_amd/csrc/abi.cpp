// abi.cpp -- extern "C" boundary: the reference's solve entry points (include/HPRLP.h) and the
// step-level extension (include/hprlp_amd.h).  Every entry point catches exceptions.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <iomanip>
#include <iostream>

#include "hprlp_amd.h"
#include "batch_prep.h"
#include "batched.h"
#include "env.h"
#include "dist.h"
#include "presolve.h"
#include "reorder.h"
#include "solver.h"
#include "stream_schedule.h"
#include "many.h"
#include "values.h"
#include "version.h"

using namespace hprlp;

struct hprlp_solver {
    Solver s;
    Comm *comm = nullptr;   // owned; destroyed after the solver's device state
    Comm *xcomm = nullptr;  // owned; the exchange stream's own communicator (second unique id), may be null
    bool sharded = false;   // created by hprlp_solver_create_dist* / _local* (no infeasibility detection)
    ~hprlp_solver() {}
};

static HPRLP_results make_error_result(const char *status) {
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

extern "C" int hprlp_warmup_seconds(double out[4]) {
    if (!out) return -1;
    for (int i = 0; i < 4; ++i) out[i] = g_warm_seconds[i];
    return 0;
}

// phases of the calling thread's last HPRLP_main_solve (hprlp_last_solve_phases): device set-up (upload, transpose, tiled
// copies, ordering), scaling, power iteration, loop, solution's way back, teardown of the device state, whole call
static thread_local double g_phases[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_solve_phases(double out[8]) {
    if (!out) return -1;
    for (int i = 0; i < 8; ++i) out[i] = g_phases[i];
    return 0;
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

// reference src/HPRLP.cu:493-524.  With use_presolve (the default) the model is first reduced on the
// host (presolve.h -- our own in-process presolver where the reference forks a PSLP worker,
// src/pslp_integration.cpp:628-713), the reduced model goes through HPRLP_main_solve and the result
// is mapped back to the original dimensions and checked against the original model
// (src/pslp_integration.cpp:715-787).  If the presolver declines, the original model is solved.
static bool is_verdict(const HPRLP_results &r) {
    return std::strcmp(r.status, "PRIMAL_INFEASIBLE") == 0 || std::strcmp(r.status, "DUAL_INFEASIBLE") == 0;
}

// solve_impl's fallback: the model as given, within what is left of the caller's time and iteration limits after `spent` seconds
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
    const auto t_entry = time_now();  // (the fallback below charges everything since here against the caller's time limit)

    // The presolver indexes its work arrays by the model's column indices and trusts rowPtr: a hand-built
    // LP_info_cpu (create_model_from_arrays validates, a caller-filled struct does not) must be refused here, before
    // any host array is touched -- without presolve DeviceMatrix::upload refuses the same models.
    if (const char *why = invalid_model_reason(model)) {
        set_last_error(why);
        std::cerr << "[error] invalid model: " << why << std::endl;
        return make_error_result("ERROR");
    }

    Presolve pre;
    bool reduced = false;
    try {
        std::cout << "Doing presolve..." << std::endl;
        reduced = pre.run(model);
        std::cout << "Presolve time: " << pre.stats().seconds << " seconds" << std::endl;
    } catch (const std::exception &e) {
        std::cerr << "[warn] presolve failed (" << e.what() << "); solving original model" << std::endl;
        reduced = false;
    }
    if (!reduced && pre.solved()) {
        // the reductions removed every row and column: the undo sequence alone produces a primal-dual optimum
        std::cout << "Presolve solved the model (no rows or columns left)" << std::endl;
        HPRLP_results r;
        std::memset(r.status, 0, sizeof(r.status));
        r.x = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
        r.y = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->m, 1)));
        r.z = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
        if (!r.x || !r.y || !r.z) {
            std::free(r.x); std::free(r.y); std::free(r.z);
            return make_error_result("ERROR");
        }
        pre.postsolve(nullptr, nullptr, nullptr, r.x, r.y, r.z);
        const OriginalKkt k = original_kkt(model, r.x, r.y, r.z);
        r.primal_obj = k.primal_obj;
        r.gap = k.gap;
        r.residuals = std::max(k.primal_feas, std::max(k.dual_feas, k.gap));
        r.time = r.time4 = r.time6 = r.time8 = pre.stats().seconds;
        r.iter = r.iter4 = r.iter6 = r.iter8 = 0;
        std::strncpy(r.status, r.residuals <= p->stop_tol ? "OPTIMAL" : "ERROR", sizeof(r.status) - 1);
        if (r.residuals <= p->stop_tol) return r;
        // (cannot happen with exact arithmetic; with rounding trouble fall back to the iteration)
        std::free(r.x); std::free(r.y); std::free(r.z);
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
    // The stopping test is relative to 1 + |b| and 1 + |c| of the model it runs on, and slack substitution moves cost
    // between columns (|c| of the reduced model can be several times the original's): the same absolute residuals would
    // then pass on the reduced model and fail the original-model check below.  Hand the reduced solve the tolerance
    // that corresponds to stop_tol on the ORIGINAL norms.
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
    norm_bc(pre.reduced(), &nb1, &nc1);
    HPRLP_parameters pr = *p;
    const double shrink = std::min(1.0, std::min((1.0 + nb0) / (1.0 + nb1), (1.0 + nc0) / (1.0 + nc1)));
    if (shrink < 1.0) {
        pr.stop_tol = p->stop_tol * shrink;
        std::cout << "Reduced-model tolerance " << pr.stop_tol << " (original norms |b| " << nb0 << ", |c| " << nc0 << "; reduced "
                  << nb1 << ", " << nc1 << ")" << std::endl;
    }
    std::vector<double> xr, yr;  // the start carried into the reduced model
    if (x0 || y0) {
        std::vector<double> xf(x0 ? x0 : nullptr, x0 ? x0 + model->n : nullptr), yf(y0 ? y0 : nullptr, y0 ? y0 + model->m : nullptr);
        xf.resize(static_cast<size_t>(model->n), 0.0);
        yf.resize(static_cast<size_t>(model->m), 0.0);
        xr.resize(static_cast<size_t>(pre.reduced()->n));
        yr.resize(static_cast<size_t>(pre.reduced()->m));
        pre.forward(xf.data(), yf.data(), xr.data(), yr.data());
    }
    HPRLP_results r = main_solve(pre.reduced(), &pr, det, cert, xr.empty() ? nullptr : xr.data(), yr.empty() ? nullptr : yr.data());
    if (det && is_verdict(r)) {
        // a certificate of the reduced model is no certificate of the caller's: solve the model as given, with detection
        std::free(r.x); std::free(r.y); std::free(r.z);
        const double spent = time_since(t_entry);
        const int it_first = r.iter;
        std::cout << "Reduced model ended " << r.status << " at iteration " << r.iter << "; solving the original model for its certificate"
                  << std::endl;
        return solve_original_rest(model, p, det, cert, x0, y0, spent, it_first);
    }
    if (det && cert) *cert = Certificate();  // (only the original model's verdicts count)
    if (!(r.x && r.y && r.z)) return r;
    double *x = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
    double *y = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->m, 1)));
    double *z = static_cast<double *>(std::malloc(sizeof(double) * std::max(model->n, 1)));
    if (!x || !y || !z) {
        std::free(x); std::free(y); std::free(z);
        std::free(r.x); std::free(r.y); std::free(r.z);
        std::cerr << "[error] out of memory in postsolve" << std::endl;
        return make_error_result("ERROR");
    }
    pre.postsolve(r.x, r.y, r.z, x, y, z);
    std::free(r.x); std::free(r.y); std::free(r.z);
    r.x = x; r.y = y; r.z = z;
    if (std::strcmp(r.status, "OPTIMAL") == 0) {
        const OriginalKkt k = original_kkt(model, x, y, z);
        const double err = std::max(k.primal_feas, std::max(k.dual_feas, k.gap));
        if (err <= p->stop_tol) {
            std::cout << "Postsolve original KKT check passed" << std::endl;
        } else {
            std::cout << "Warning: postsolve original KKT check failed (the primal solution and objective are reliable)\n"
                      << "  Primal Residual: " << k.primal_feas << "  Dual Residual: " << k.dual_feas
                      << "  Relative Gap: " << k.gap << "  (tolerance " << p->stop_tol << ")" << std::endl;
            // Safety net: a reduced model that is solved to tolerance but misses the original model by orders of magnitude
            // means a reduction went wrong on this input -- solve the model as given rather than hand back a wrong answer.
            if (err > 100.0 * p->stop_tol && err > 1e-3) {
                std::cout << "Postsolved solution is far from the original model's KKT conditions; solving the original model" << std::endl;
                std::free(r.x); std::free(r.y); std::free(r.z);
                const double spent = time_since(t_entry);
                const int it_first = r.iter;
                HPRLP_results r2 = solve_original_rest(model, p, det, cert, x0, y0, spent, it_first);
                std::cout << "Fallback solve: reported time and iterations include presolve and the reduced solve (" << spent
                          << " s, " << it_first << " iterations)" << std::endl;
                return r2;
            }
        }
    } else {
        std::cout << "Skipping postsolve original KKT check since the reduced solution is not optimal" << std::endl;
    }
    return r;
}

extern "C" HPRLP_results solve(const LP_info_cpu *model, const HPRLP_parameters *param) {
    return solve_impl(model, param, nullptr, nullptr);
}

static void clear_certificate(hprlp_certificate *c, int m, int n) {
    std::memset(c, 0, sizeof(*c));
    c->m = m;
    c->n = n;
}

// Certificate -> hprlp_certificate (malloc'd arrays); false when the host allocation failed
static bool export_certificate(const Certificate &k, hprlp_certificate *c, int m, int n) {
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

static bool detection_from(const hprlp_detection *d, Detection *out) {
    if (!d) return false;
    if (!(d->eps_primal_infeasible >= 0.0) || !(d->eps_dual_infeasible >= 0.0))
        throw std::runtime_error("infeasibility detection: eps_primal_infeasible and eps_dual_infeasible must be >= 0");
    out->on = true;
    out->eps_primal = d->eps_primal_infeasible;
    out->eps_dual = d->eps_dual_infeasible;
    return true;
}

// a warm start's entries must be finite (null: zeros)
static void check_start(const double *v, long len, const char *what) {
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
            std::free(r.x); std::free(r.y); std::free(r.z);
            throw std::runtime_error("host allocation of the certificate failed");
        }
        return r;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        std::cerr << "[error] " << who << " failed: " << e.what() << std::endl;
        return make_error_result("ERROR");
    }
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

// sizes and zeroed per-member arrays (kind 0 for every member), no ray arrays; false when the host allocation failed
static bool clear_batched_certificates(hprlp_batched_certificates *c, int B, int m, int n) {
    std::memset(c, 0, sizeof(*c));
    c->batch_size = B;
    c->m = m;
    c->n = n;
    if (B <= 0) return true;
    c->kind = static_cast<int *>(std::calloc(B, sizeof(int)));
    c->iter = static_cast<int *>(std::calloc(B, sizeof(int)));
    c->objective = static_cast<double *>(std::calloc(B, sizeof(double)));
    c->violation = static_cast<double *>(std::calloc(B, sizeof(double)));
    return c->kind && c->iter && c->objective && c->violation;
}

// one Certificate per member -> column-major arrays (a member's columns stay zero where its kind does not use them)
static bool export_batched_certificates(const std::vector<Certificate> &k, hprlp_batched_certificates *c) {
    const int B = c->batch_size;
    const size_t m = static_cast<size_t>(c->m), n = static_cast<size_t>(c->n);
    bool any_y = false, any_d = false;
    for (int j = 0; j < B && j < static_cast<int>(k.size()); ++j) {
        c->kind[j] = k[j].kind;
        c->iter[j] = k[j].iter;
        c->objective[j] = k[j].objective;
        c->violation[j] = k[j].violation;
        any_y = any_y || k[j].kind == 1;
        any_d = any_d || k[j].kind == 2;
    }
    auto panel = [B](size_t rows, double **out) {
        *out = static_cast<double *>(std::calloc(std::max<size_t>(rows * B, 1), sizeof(double)));
        return *out != nullptr;
    };
    if ((any_y && (!panel(m, &c->y) || !panel(n, &c->z))) || (any_d && !panel(n, &c->d))) return false;
    for (int j = 0; j < B && j < static_cast<int>(k.size()); ++j) {
        if (k[j].kind == 1) {
            std::memcpy(c->y + j * m, k[j].y.data(), sizeof(double) * m);
            std::memcpy(c->z + j * n, k[j].z.data(), sizeof(double) * n);
        } else if (k[j].kind == 2) {
            std::memcpy(c->d + j * n, k[j].d.data(), sizeof(double) * n);
        }
    }
    return true;
}

// hprlp_solve_batched_detect and hprlp_solve_batched_warm (`who`, for the error messages), as solve_entry: no detection and no
// starts are exactly solve_batched(); the certificates are cleared on entry and filled only when detection ran
static HPRLP_batched_results solve_batched_entry(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                                 const double *AU, const double *l, const double *u, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *X0, const double *Y0,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs, const char *who) {
    const int m = model ? model->m : 0, n = model ? model->n : 0, B = std::max(batch_size, 0);
    const bool warm = X0 || Y0;
    try {
        if (certs && !clear_batched_certificates(certs, B, m, n)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        if (!det && !warm) return solve_batched(model, batch_size, C, AL, AU, l, u, obj_constants, param);
        if (warm) {
            if (!model) throw std::runtime_error("null model");
            check_start(X0, static_cast<long>(n) * B, "X0");
            check_start(Y0, static_cast<long>(m) * B, "Y0");
        }
        Detection d;
        const bool with_det = detection_from(det, &d);
        std::vector<Certificate> k;
        HPRLP_batched_results r = solve_batched_impl(model, batch_size, C, AL, AU, l, u, obj_constants, param, with_det ? &d : nullptr,
                                                     with_det && certs ? &k : nullptr, X0, Y0);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            free_batched_results(&r);
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        return r;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        std::cerr << "[error] " << who << " failed: " << e.what() << std::endl;
        return make_batched_error("ERROR", m, n, B);
    }
}

extern "C" HPRLP_batched_results hprlp_solve_batched_detect(const LP_info_cpu *model, int batch_size, const double *C,
                                                            const double *AL, const double *AU, const double *l, const double *u,
                                                            const double *obj_constants, const HPRLP_parameters *param,
                                                            const hprlp_detection *det, hprlp_batched_certificates *certs) {
    return solve_batched_entry(model, batch_size, C, AL, AU, l, u, obj_constants, param, nullptr, nullptr, det, certs,
                               "hprlp_solve_batched_detect");
}

extern "C" HPRLP_batched_results hprlp_solve_batched_warm(const LP_info_cpu *model, int batch_size, const double *C, const double *AL,
                                                          const double *AU, const double *l, const double *u,
                                                          const double *obj_constants, const HPRLP_parameters *param,
                                                          const double *X0, const double *Y0, const hprlp_detection *det,
                                                          hprlp_batched_certificates *certs) {
    if (!X0 && !Y0) return hprlp_solve_batched_detect(model, batch_size, C, AL, AU, l, u, obj_constants, param, det, certs);
    return solve_batched_entry(model, batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, det, certs,
                               "hprlp_solve_batched_warm");
}

// ---- resident batches (DESIGN.md "Resident batches"): a sequence of batches over one matrix ------------------------------------
struct hprlp_batched_solver {
    BatchedSolver *s = nullptr;
};

extern "C" hprlp_batched_solver *hprlp_batched_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param) {
    hprlp_batched_solver *h = nullptr;
    try {
        if (!model || !model->A) throw std::runtime_error("hprlp_batched_solver_create: null model");
        int count = 0;
        if (hipInit(0) != hipSuccess || hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
            (void)hipGetLastError();
            throw std::runtime_error("hprlp_batched_solver_create: no usable GPU");
        }
        h = new hprlp_batched_solver();
        h->s = batched_solver_create(model, param);
        return h;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        delete h;
        return nullptr;
    }
}

extern "C" void hprlp_batched_solver_destroy(hprlp_batched_solver *h) {
    if (!h) return;
    batched_solver_destroy(h->s);
    delete h;
}

extern "C" int hprlp_batched_solver_solve(hprlp_batched_solver *h, int batch_size, const double *C, const double *AL, const double *AU,
                                          const double *l, const double *u, const double *obj_constants, const HPRLP_parameters *param,
                                          const double *X0, const double *Y0, int carry, const hprlp_detection *det,
                                          hprlp_batched_certificates *certs, HPRLP_batched_results *out) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_solve: null solver");
        if (!out) throw std::runtime_error("hprlp_batched_solver_solve: null results");
        long mn[8];
        batched_solver_info(h->s, mn);
        const int m = static_cast<int>(mn[0]), n = static_cast<int>(mn[1]), B = std::max(batch_size, 0);
        if (certs && !clear_batched_certificates(certs, B, m, n)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        check_start(X0, static_cast<long>(n) * B, "X0");
        check_start(Y0, static_cast<long>(m) * B, "Y0");
        Detection d;
        const bool with_det = detection_from(det, &d);
        std::vector<Certificate> k;
        HPRLP_batched_results r;
        batched_solver_solve(h->s, batch_size, C, AL, AU, l, u, obj_constants, param, X0, Y0, carry != 0, with_det ? &d : nullptr,
                             with_det && certs ? &k : nullptr, &r);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            free_batched_results(&r);
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// ---- streamed batches (DESIGN.md "Streamed batches") ---------------------------------------------------------------------------
// What can be told from the arguments alone is refused first, so that those refusals need no solver (and no GPU).
extern "C" int hprlp_batched_solver_solve_stream(hprlp_batched_solver *h, int count, int width, const double *C, const double *AL,
                                                 const double *AU, const double *l, const double *u, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *X0, const double *Y0,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs,
                                                 HPRLP_batched_results *out) {
    bool certs_cleared = false;  // (a call that fails after this leaves no allocation behind in certs)
    try {
        // (with param NULL the solver's own parameters decide, and the solver asks again)
        stream_check_call(out != nullptr, count, width, C && AL && AU && l && u, param ? param->max_iter : 0, param ? param->check_iter : 1);
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_solve_stream: null solver");
        long mn[8];
        batched_solver_info(h->s, mn);
        const int m = static_cast<int>(mn[0]), n = static_cast<int>(mn[1]);
        Detection d;  // (the starts' finite entries: the solver checks them, before it changes)
        const bool with_det = detection_from(det, &d);
        certs_cleared = certs != nullptr;
        if (certs && !clear_batched_certificates(certs, count, m, n)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        std::vector<Certificate> k;
        HPRLP_batched_results r;
        batched_solver_solve_stream(h->s, count, width, C, AL, AU, l, u, obj_constants, param, X0, Y0, with_det ? &d : nullptr,
                                    with_det && certs ? &k : nullptr, &r);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            free_batched_results(&r);
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        if (certs_cleared) hprlp_free_batched_certificates(certs);
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_stream_record(hprlp_batched_solver *h, int *slot, int *event_in, int *event_out) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_stream_record: null solver");
        return batched_solver_stream_record(h->s, slot, event_in, event_out);
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_stream_info(hprlp_batched_solver *h, long out[8]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_stream_info: null solver / output");
        batched_solver_stream_info(h->s, out, nullptr);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_stream_seconds(hprlp_batched_solver *h, double out[2]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_stream_seconds: null solver / output");
        long counts[8];
        batched_solver_stream_info(h->s, counts, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_lambda(hprlp_batched_solver *h, double out[2]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_lambda: null solver / output");
        batched_solver_lambda(h->s, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_stream_schedule_host(int count, int width, const int *events, int *slot, int *event_in, int *event_out) {
    try {
        return stream_schedule(count, width, events, slot, event_in, event_out);
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_solve_device(hprlp_batched_solver *h, int batch_size, const double *dC, const double *dAL,
                                                 const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                                 const HPRLP_parameters *param, const double *dX0, const double *dY0, int carry,
                                                 const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                                 double *dx, double *dy, double *dz, hprlp_batched_scalars *out) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_solve_device: null solver");
        if (!out) throw std::runtime_error("hprlp_batched_solver_solve_device: null scalars");
        long mn[8];
        batched_solver_info(h->s, mn);
        const int m = static_cast<int>(mn[0]), n = static_cast<int>(mn[1]), B = std::max(batch_size, 0);
        if (certs && !clear_batched_certificates(certs, B, m, n)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        Detection d;
        const bool with_det = detection_from(det, &d);
        std::vector<Certificate> k;
        DeviceBatch db;
        db.stream = stream;
        db.x = dx; db.y = dy; db.z = dz;
        db.primal_obj = out->primal_obj; db.residuals = out->residuals; db.gap = out->gap; db.iter = out->iter; db.status = out->status;
        if (out->status && B > 0) std::memset(out->status, 0, static_cast<size_t>(B) * 64);
        batched_solver_solve_device(h->s, batch_size, dC, dAL, dAU, dl, du, obj_constants, param, dX0, dY0, carry != 0,
                                    with_det ? &d : nullptr, with_det && certs ? &k : nullptr, &db);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        out->time = db.time; out->setup_time = db.setup_time; out->solve_time = db.solve_time; out->power_time = db.power_time;
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// ---- device-resident streams (DESIGN.md "Device-resident streams") -----------------------------------------------------------------
// As the host stream: what the arguments alone tell is refused first, with its words, and needs no solver.
extern "C" int hprlp_batched_solver_solve_stream_device(hprlp_batched_solver *h, int count, int width, const double *dC, const double *dAL,
                                                        const double *dAU, const double *dl, const double *du, const double *obj_constants,
                                                        const HPRLP_parameters *param, const double *dX0, const double *dY0,
                                                        const hprlp_detection *det, hprlp_batched_certificates *certs, void *stream,
                                                        double *dx, double *dy, double *dz, hprlp_batched_scalars *out) {
    bool certs_cleared = false;
    try {
        stream_check_call(out && dx && dy && dz, count, width, dC && dAL && dAU && dl && du, param ? param->max_iter : 0,
                          param ? param->check_iter : 1);
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_solve_stream_device: null solver");
        long mn[8];
        batched_solver_info(h->s, mn);
        const int m = static_cast<int>(mn[0]), n = static_cast<int>(mn[1]);
        Detection d;
        const bool with_det = detection_from(det, &d);
        certs_cleared = certs != nullptr;
        if (certs && !clear_batched_certificates(certs, count, m, n)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        std::vector<Certificate> k;
        DeviceBatch db;
        db.stream = stream;
        db.x = dx; db.y = dy; db.z = dz;
        db.primal_obj = out->primal_obj; db.residuals = out->residuals; db.gap = out->gap; db.iter = out->iter; db.status = out->status;
        if (out->status) std::memset(out->status, 0, static_cast<size_t>(count) * 64);
        batched_solver_solve_stream_device(h->s, count, width, dC, dAL, dAU, dl, du, obj_constants, param, dX0, dY0, with_det ? &d : nullptr,
                                           with_det && certs ? &k : nullptr, &db);
        if (with_det && certs && !export_batched_certificates(k, certs)) {
            hprlp_free_batched_certificates(certs);
            throw std::runtime_error("host allocation of the certificates failed");
        }
        out->time = db.time; out->setup_time = db.setup_time; out->solve_time = db.solve_time; out->power_time = db.power_time;
        return 0;
    } catch (const std::exception &e) {
        if (certs_cleared) hprlp_free_batched_certificates(certs);
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_stream_memory(hprlp_batched_solver *h, long out[4]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_stream_memory: null solver / output");
        batched_solver_stream_memory(h->s, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_set_norms(hprlp_batched_solver *h, int rule) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_set_norms: null solver");
        batched_solver_set_norms(h->s, rule);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_scalars(hprlp_batched_solver *h, double *out) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_scalars: null solver / output");
        return batched_solver_scalars(h->s, out);
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_transfer(hprlp_batched_solver *h, long out[4]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_transfer: null solver / output");
        batched_solver_transfer(h->s, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_info(hprlp_batched_solver *h, long out[8]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_info: null solver / output");
        batched_solver_info(h->s, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_seconds(hprlp_batched_solver *h, double out[6]) {
    try {
        if (!h || !h->s || !out) throw std::runtime_error("hprlp_batched_solver_seconds: null solver / output");
        batched_solver_seconds(h->s, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// One ray test outside the loop on the resident batched solver, and its panels by name (batched.hip: batched_solver_ray_step)
extern "C" int hprlp_batched_solver_ray_step(hprlp_batched_solver *h, const int *active, int restart, double *out, int *tested) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_ray_step: null solver");
        return batched_solver_ray_step(h->s, active, restart != 0, out, tested);
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" long hprlp_batched_solver_get_panel(hprlp_batched_solver *h, const char *name, double *out, long len) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_get_panel: null solver");
        return batched_solver_get_panel(h->s, name, out, len);
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_batched_solver_set_panel(hprlp_batched_solver *h, const char *name, const double *in, long len) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_set_panel: null solver");
        batched_solver_set_panel(h->s, name, in, len);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" void hprlp_free_batched_certificates(hprlp_batched_certificates *certs) {
    if (!certs) return;
    for (void *p : {static_cast<void *>(certs->kind), static_cast<void *>(certs->iter), static_cast<void *>(certs->objective),
                    static_cast<void *>(certs->violation), static_cast<void *>(certs->y), static_cast<void *>(certs->z),
                    static_cast<void *>(certs->d)})
        std::free(p);
    certs->kind = certs->iter = nullptr;
    certs->objective = certs->violation = certs->y = certs->z = certs->d = nullptr;
}

// presolve as separate steps (host only; used by the CPU tests and by callers that want the maps)
struct hprlp_presolve {
    Presolve p;
};
extern "C" hprlp_presolve *hprlp_presolve_run(const LP_info_cpu *model) {
    hprlp_presolve *h = nullptr;
    try {
        h = new hprlp_presolve();
        if (h->p.run(model)) return h;
        set_last_error("presolve left the model unchanged");
    } catch (const std::exception &e) {
        set_last_error(e.what());
    }
    delete h;
    return nullptr;
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

// ------------------------------------------------------------------------------------------------
// step-level extension
// ------------------------------------------------------------------------------------------------
#define GUARD_BEGIN try {
#define GUARD_END(failval)                    \
    }                                         \
    catch (const std::exception &e) {         \
        set_last_error(e.what());             \
        return failval;                       \
    }

extern "C" hprlp_solver *hprlp_solver_create(const LP_info_cpu *model, const HPRLP_parameters *param) {
    if (!model) {
        set_last_error("null model");
        return nullptr;
    }
    hprlp_solver *h = nullptr;
    try {
        HPRLP_parameters dflt;
        h = new hprlp_solver();
        h->s.verbose = false;
        h->s.setup(model, param ? param : &dflt);
        return h;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        delete h;
        return nullptr;
    }
}

struct hprlp_local_group {
    LocalGroup *g = nullptr;
};
extern "C" hprlp_local_group *hprlp_local_group_create(int size) {
    try {
        auto *h = new hprlp_local_group();
        h->g = make_local_group(size);
        return h;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return nullptr;
    }
}
extern "C" void hprlp_local_group_destroy(hprlp_local_group *h) {
    if (!h) return;
    free_local_group(h->g);
    delete h;
}

// A launcher that hands over TWO unique ids (256 bytes, hprlp_dist_unique_id with a 256-byte buffer) gets a second
// communicator for the exchange stream: the exchanges that overlap the local part of a half-step are enqueued on another
// stream than the collectives of the check iterations, and one RCCL communicator must not be driven from two streams.
static void make_exchange_comm(hprlp_solver *h, int rank, int size, const void *unique_id, int id_bytes, int device) {
    if (!unique_id || id_bytes < 256) return;
    // a launcher that padded ONE id to 256 bytes: bytes 128..255 hold no id -- single communicator (the documented fallback)
    bool any = false;
    for (int k = 128; k < 256; ++k) any = any || static_cast<const unsigned char *>(unique_id)[k] != 0;
    if (!any) return;
    h->xcomm = make_rccl_comm(rank, size, static_cast<const char *>(unique_id) + 128, 128, device);
    h->s.xcomm = h->xcomm;
}

// The transport a (rank, size, id) names: a shared-memory group of processes (id made under HPRLP_DIST_TRANSPORT=shm; staging
// room = one full-length vector per rank) or RCCL communicators (one, or two when the launcher handed over two ids).
static void make_transport(hprlp_solver *h, int m, int n, int rank, int size, const void *unique_id, int id_bytes, int device) {
    if (is_shm_unique_id(unique_id, static_cast<size_t>(id_bytes))) {
        const size_t area = (static_cast<size_t>(std::max(m, n)) + 64u * static_cast<size_t>(size)) * sizeof(double) + 4096u * static_cast<size_t>(size + 1);
        h->comm = make_shm_comm(rank, size, unique_id, static_cast<size_t>(id_bytes), area, device);
        return;
    }
    h->comm = make_rccl_comm(rank, size, unique_id, static_cast<size_t>(id_bytes), device);
    make_exchange_comm(h, rank, size, unique_id, id_bytes, device);
}

static void destroy_handle(hprlp_solver *h) {
    if (!h) return;
    Comm *c = h->comm, *x = h->xcomm;
    delete h;  // the solver first: its device state (and a background tiling job) goes before the transport
    delete x;
    delete c;
}

// rank `rank` of `size`: RCCL communicator from unique_id, or (group != NULL) the in-process group
static hprlp_solver *create_sharded(const LP_info_cpu *model, const HPRLP_parameters *param, int rank, int size,
                                    const void *unique_id, int id_bytes, hprlp_local_group *group) {
    if (!model) {
        set_last_error("null model");
        return nullptr;
    }
    hprlp_solver *h = nullptr;
    hprlp_shard sh;
    std::memset(&sh, 0, sizeof(sh));
    try {
        HPRLP_parameters dflt;
        const HPRLP_parameters *p = param ? param : &dflt;
        if (hprlp_extract_shard(model, rank, size, &sh) != 0) throw std::runtime_error(last_error_cstr());
        h = new hprlp_solver();
        h->sharded = true;
        h->s.verbose = false;
        HIP_CHECK(hipSetDevice(p->device_number));
        if (group) {
            h->comm = make_local_comm(group->g, rank);
        } else if (size > 1 || (unique_id && id_bytes >= 128)) {
            // a unique id given with size 1 builds a one-rank RCCL communicator (exercises the collective path)
            make_transport(h, sh.m, sh.n, rank, size, unique_id, id_bytes, p->device_number);
        }
        h->s.setup_shard(sh.m, sh.n, sh.row_off, sh.m_loc, sh.col_off, sh.n_loc, sh.A_rowptr, sh.A_col, sh.A_val,
                         sh.AT_rowptr, sh.AT_col, sh.AT_val, sh.AL, sh.AU, sh.l, sh.u, sh.c, sh.obj_constant, p, h->comm);
        hprlp_free_shard(&sh);
        return h;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        destroy_handle(h);  // the solver first: a background tiling job may still read the shard arrays (its destructor joins it)
        hprlp_free_shard(&sh);
        return nullptr;
    }
}

extern "C" hprlp_solver *hprlp_solver_create_dist(const LP_info_cpu *model, const HPRLP_parameters *param, int rank,
                                                  int size, const void *unique_id, int id_bytes) {
    return create_sharded(model, param, rank, size, unique_id, id_bytes, nullptr);
}

// The same from a shard the caller built itself (no rank ever holds the whole matrix: SURVEY.md 8d, config 5 "generated per
// shard"); the shard stays the caller's.
static hprlp_solver *create_from_shard(const hprlp_shard *sh, const HPRLP_parameters *param, int rank, int size, const void *unique_id,
                                       int id_bytes, hprlp_local_group *group) {
    hprlp_solver *h = nullptr;
    try {
        if (!sh || !sh->A_rowptr || !sh->AT_rowptr || (sh->m_loc > 0 && !(sh->AL && sh->AU)) || (sh->n_loc > 0 && !(sh->l && sh->u && sh->c)))
            throw std::runtime_error("incomplete shard");
        if (sh->A_rowptr[sh->m_loc] > 0 && !(sh->A_col && sh->A_val)) throw std::runtime_error("incomplete shard (A)");
        if (sh->AT_rowptr[sh->n_loc] > 0 && !(sh->AT_col && sh->AT_val)) throw std::runtime_error("incomplete shard (A^T)");
        HPRLP_parameters dflt;
        const HPRLP_parameters *p = param ? param : &dflt;
        h = new hprlp_solver();
        h->sharded = true;
        h->s.verbose = false;
        HIP_CHECK(hipSetDevice(p->device_number));
        if (group) h->comm = make_local_comm(group->g, rank);
        else if (size > 1 || (unique_id && id_bytes >= 128)) {
            make_transport(h, sh->m, sh->n, rank, size, unique_id, id_bytes, p->device_number);
        }
        h->s.setup_shard(sh->m, sh->n, sh->row_off, sh->m_loc, sh->col_off, sh->n_loc, sh->A_rowptr, sh->A_col, sh->A_val, sh->AT_rowptr,
                         sh->AT_col, sh->AT_val, sh->AL, sh->AU, sh->l, sh->u, sh->c, sh->obj_constant, p, h->comm);
        return h;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        destroy_handle(h);
        return nullptr;
    }
}

extern "C" hprlp_solver *hprlp_solver_create_dist_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                             const void *unique_id, int id_bytes) {
    return create_from_shard(shard, param, rank, size, unique_id, id_bytes, nullptr);
}

extern "C" hprlp_solver *hprlp_solver_create_local_from_shard(const hprlp_shard *shard, const HPRLP_parameters *param, int rank, int size,
                                                              hprlp_local_group *group) {
    if (!group) {
        set_last_error("null local group");
        return nullptr;
    }
    return create_from_shard(shard, param, rank, size, nullptr, 0, group);
}

extern "C" hprlp_solver *hprlp_solver_create_local(const LP_info_cpu *model, const HPRLP_parameters *param, int rank,
                                                   int size, hprlp_local_group *group) {
    if (!group) {
        set_last_error("null local group");
        return nullptr;
    }
    return create_sharded(model, param, rank, size, nullptr, 0, group);
}

// The shared-memory transport's protocol on HOST buffers (no GPU, no HIP call): rank `rank` of `size` attaches to the group the
// id names and runs `rounds` rounds of all-gather, scalar all-reduce and a neighbour exchange whose payloads every receiver
// checks.  hang_rank >= 0: that rank leaves before round `rounds / 2` without a word (the others must end with an error once
// HPRLP_DIST_TIMEOUT_S has passed, not wait for ever).  Returns 0, or -1 + hprlp_last_error().
extern "C" int hprlp_shm_transport_selftest(const void *unique_id, int id_bytes, int rank, int size, int rounds, int hang_rank) {
    try {
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
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// out = {halo_m sparse?, entries sent, entries received, halo_n sparse?, sent, received, requests m, requests n}
extern "C" int hprlp_solver_dist_info(hprlp_solver *h, long out[8]) {
    if (!h || !out) return -1;
    const Solver &s = h->s;
    out[0] = s.halo_m.sparse; out[1] = s.halo_m.nsend; out[2] = s.halo_m.nrecv;
    out[3] = s.halo_n.sparse; out[4] = s.halo_n.nsend; out[5] = s.halo_n.nrecv;
    out[6] = s.halo_m.total_requests; out[7] = s.halo_n.total_requests;
    return 0;
}

// out = {ranks / this rank / device as the main communicator reports them (RCCL: ncclCommCount, ncclCommUserRank,
//        ncclCommCuDevice), the same three of the exchange stream's communicator (0, -1, -1 if there is none), the
//        solver's HIP device, 1 if the exchange overlaps the local part of the half-steps}
extern "C" int hprlp_solver_dist_comm_info(hprlp_solver *h, long out[8]) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("null solver / output");
    const Solver &s = h->s;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[1] = out[2] = out[4] = out[5] = -1;
    if (s.comm) { out[0] = s.comm->reported_ranks(); out[1] = s.comm->reported_rank(); out[2] = s.comm->reported_device(); }
    if (s.xcomm) { out[3] = s.xcomm->reported_ranks(); out[4] = s.xcomm->reported_rank(); out[5] = s.xcomm->reported_device(); }
    out[6] = s.prm.device_number;
    out[7] = s.overlap_enabled ? 1 : 0;
    return 0;
    GUARD_END(-1)
}

// One grouped send/recv of `count` doubles from this rank to ITSELF through the solver's communicator (pattern
// i -> 3 i + 1), checked on the host: exercises the point-to-point entry points of the transport (RCCL: ncclGroupStart /
// ncclSend / ncclRecv / ncclGroupEnd) on a box where no second rank can exist.  0 = delivered intact.
extern "C" int hprlp_solver_dist_loopback(hprlp_solver *h, int count) {
    GUARD_BEGIN
    Solver &s = h->s;
    if (!s.comm) throw std::runtime_error("solver has no communicator");
    if (count <= 0) throw std::runtime_error("count must be positive");
    std::vector<double> src(static_cast<size_t>(count)), dst(static_cast<size_t>(count), -1.0);
    for (int i = 0; i < count; ++i) src[i] = 3.0 * i + 1.0;
    DBuf<double> a(src.size()), b(dst.size());
    a.upload(src.data(), src.size());
    b.upload(dst.data(), dst.size());
    const P2P op{s.comm->rank, a.p, src.size() * sizeof(double), b.p, dst.size() * sizeof(double)};
    s.comm->exchange(&op, 1, s.stream);
    HIP_CHECK(hipStreamSynchronize(s.stream));
    b.download(dst.data(), dst.size());
    for (int i = 0; i < count; ++i)
        if (dst[i] != src[i]) throw std::runtime_error("loopback send/recv delivered wrong data at element " + std::to_string(i));
    return 0;
    GUARD_END(-1)
}

extern "C" void hprlp_solver_destroy(hprlp_solver *h) {
    try {
        destroy_handle(h);
    } catch (...) {
    }
}

extern "C" void hprlp_solver_set_verbose(hprlp_solver *h, int verbose) {
    if (h) h->s.verbose = verbose != 0;
}

extern "C" int hprlp_solver_scale(hprlp_solver *h) {
    GUARD_BEGIN
    h->s.scale();
    return 0;
    GUARD_END(-1)
}

extern "C" double hprlp_solver_power_iteration(hprlp_solver *h, int max_iter, double tol, int *iters_out) {
    GUARD_BEGIN
    return h->s.power_iteration(max_iter, tol, iters_out);
    GUARD_END(-1.0)
}

extern "C" int hprlp_solver_init(hprlp_solver *h, double sigma, double lambda_max) {
    GUARD_BEGIN
    h->s.lambda_max = lambda_max;
    if (sigma > 0) h->s.set_sigma_lambda(sigma, lambda_max, true);
    else h->s.init_iteration_state();
    HIP_CHECK(hipStreamSynchronize(h->s.stream));
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_reset_iterates(hprlp_solver *h) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("null solver");
    h->s.reset_iterates();
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_iterate(hprlp_solver *h, int normal, int then_check) {
    GUARD_BEGIN
    if (then_check) h->s.run_normal_then_check(normal);
    else h->s.run_normal(normal);
    HIP_CHECK(hipStreamSynchronize(h->s.stream));
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_residuals(hprlp_solver *h, int iter, int compute_gap, double out[8]) {
    GUARD_BEGIN
    Residuals r;
    RestartState rs;
    h->s.compute_residuals(iter, compute_gap != 0, &r, &rs);
    out[0] = r.err_Rp; out[1] = r.err_Rd; out[2] = r.primal_obj; out[3] = r.dual_obj;
    out[4] = r.rel_gap; out[5] = r.kkt; out[6] = rs.current_gap; out[7] = h->s.lambda_max;
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_restart(hprlp_solver *h, const double in[6], double *sigma_out) {
    GUARD_BEGIN
    RestartState rs;
    rs.flag = 1;
    rs.first = false;
    rs.current_gap = in[0]; rs.best_gap = in[1]; rs.best_sigma = in[2];
    Residuals r;
    r.err_Rd = in[3]; r.err_Rp = in[4]; r.rel_gap = in[5];
    h->s.update_sigma_and_restart(&rs, r);
    HIP_CHECK(hipStreamSynchronize(h->s.stream));
    if (sigma_out) *sigma_out = h->s.sigma;
    return 0;
    GUARD_END(-1)
}

extern "C" double hprlp_solver_weighted_norm(hprlp_solver *h) {
    GUARD_BEGIN
    return h->s.weighted_norm_after_restart();
    GUARD_END(-1.0)
}

extern "C" int hprlp_solver_run(hprlp_solver *h, HPRLP_results *out, hprlp_trace_row *trace, int max_trace,
                                int *n_trace) {
    GUARD_BEGIN
    static_assert(sizeof(hprlp_trace_row) == sizeof(TraceRow), "trace row layout");
    h->s.trace = reinterpret_cast<TraceRow *>(trace);
    h->s.trace_cap = trace ? max_trace : 0;
    h->s.solve_loop(out);
    h->s.collect_solution(out);
    if (n_trace) *n_trace = h->s.trace_n;
    h->s.trace = nullptr;
    h->s.trace_cap = 0;
    return 0;
    GUARD_END(-1)
}

// ------------------------------------------------------------------------------------------------
// many small LPs at once (many.cpp; DESIGN.md "Many small LPs")
// ------------------------------------------------------------------------------------------------
// the members of a group call, checked before anything is launched (`who`, for the error messages)
static std::vector<Solver *> group_members(hprlp_solver **h, int count, const char *who, bool need_scaled = true) {
    const std::string w(who);
    if (!h) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    std::vector<Solver *> s(static_cast<size_t>(count));
    for (int k = 0; k < count; ++k) {
        if (!h[k]) throw std::runtime_error(w + ": member " + std::to_string(k) + " is null");
        if (h[k]->sharded)
            throw std::runtime_error(w + ": member " + std::to_string(k) + " is a sharded solver (hprlp_solver_create_dist* / _local*); a group runs on one GPU");
        s[k] = &h[k]->s;
    }
    check_group(s.data(), count, who, need_scaled);
    return s;
}
// the refusals of a group entry's plain arguments, in their order: the list, the count, then `arg` (data or results, `what` in the
// message); group_members comes next
static void check_group_args(hprlp_solver **h, int count, const void *arg, const char *what, const char *who) {
    const std::string w(who);
    if (!h) throw std::runtime_error(w + ": null solver list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    if (!arg) throw std::runtime_error(w + ": null " + what);
}

// the public member structs as many.h's
static MemberData to_private(const hprlp_member_data &d) {
    MemberData r;
    r.c = d.c, r.obj_constant = d.obj_constant, r.AL = d.AL, r.AU = d.AU, r.l = d.l, r.u = d.u;
    return r;
}
static MemberValues to_private(const hprlp_member_values &d) {
    MemberValues r;
    r.val = d.val, r.nnz = d.nnz, r.c = d.c, r.obj_constant = d.obj_constant, r.AL = d.AL, r.AU = d.AU, r.l = d.l, r.u = d.u;
    return r;
}
static MemberStart to_private(const hprlp_member_start &b) {
    MemberStart r;
    r.x0 = b.x0, r.y0 = b.y0, r.sigma = b.sigma;
    return r;
}
static MemberOut to_private(const hprlp_member_out &o) {
    MemberOut r;
    r.x = o.x, r.y = o.y, r.z = o.z;
    return r;
}
// one private struct per member; a null list: every member's default (a cold start, no output wanted)
template <class Private, class Public>
static std::vector<Private> private_members(const Public *list, int count) {
    std::vector<Private> v(static_cast<size_t>(count));
    for (int k = 0; list && k < count; ++k) v[k] = to_private(list[k]);
    return v;
}

// The count blocks of the group calls: eight slots each, the calling thread's own, filled by keep_counts and read by the
// hprlp_last_*_counts accessors.  Which call zeroes which block, and when, is the call's own business (tests read it).
static void keep_counts(long (&block)[8], const long (&v)[8]) {
    for (int i = 0; i < 8; ++i) block[i] = v[i];
}
static int read_counts(const long (&block)[8], long out[8]) {
    if (!out) return -1;
    for (int i = 0; i < 8; ++i) out[i] = block[i];
    return 0;
}

// ---- group set-up, scaling and teardown (DESIGN.md "Many small LPs", group set-up) -------------------------------------------
// counts of the calling thread's last hprlp_solver_create_many / _scale_many / _destroy_many; each call zeroes and fills its own
static thread_local long g_setup_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_setup_many_counts(long out[8]) { return read_counts(g_setup_counts, out); }

// hprlp_solver_create for every model.  together: the members whose set-up only allocates, zeroes and uploads
// (Solver::group_setup_fits) are created inside one arena -- a few device blocks, one pinned block, one stream, one copy per
// block and one wait for all of them; every other member, and everybody when !together, is set up as hprlp_solver_create does.
// A model that fails leaves out[k] = NULL and its message in hprlp_last_error(); the others are created.  Returns the number
// created.
static int create_group(const LP_info_cpu *const *models, int count, const HPRLP_parameters *p, hprlp_solver **out, const char *who, bool together) {
    for (int k = 0; k < count; ++k) out[k] = nullptr;
    const AllocCounts before = alloc_counts();
    Arena *arena = nullptr;
    if (together) {
        try {
            arena = arena_create(p->device_number);
        } catch (const std::exception &) {
            // (no device, a wrong device number: every member says so itself below, as in a set-up member by member)
        }
    }
    struct CreatorsReference {  // (the members hold their own: the arena goes with the last of them, or here if nobody joined it)
        Arena *a;
        ~CreatorsReference() { arena_release(a); }
    } creators{arena};
    int made = 0;
    try {
        for (int k = 0; k < count; ++k) {
            hprlp_solver *h = nullptr;
            try {
                if (!models[k]) throw std::runtime_error("null model");
                h = new hprlp_solver();
                h->s.verbose = false;
                if (arena && Solver::group_setup_fits(models[k])) {
                    ArenaScope scope(arena);
                    h->s.setup(models[k], p);
                } else {
                    h->s.setup(models[k], p);
                }
                out[k] = h;
                ++made;
            } catch (const std::exception &e) {
                set_last_error(std::string(who) + ": model " + std::to_string(k) + ": " + e.what());
                std::cerr << "[error] " << who << ": model " << k << " failed its set-up: " << e.what() << std::endl;
                delete h;
            }
        }
        if (arena) arena_flush(arena);
        if (made > 0) HIP_CHECK(hipDeviceSynchronize());
    } catch (...) {
        for (int k = 0; k < count; ++k) {
            delete out[k];
            out[k] = nullptr;
        }
        throw;
    }
    const AllocCounts after = alloc_counts();
    g_setup_counts[0] = after.device_allocs - before.device_allocs;
    g_setup_counts[1] = after.pinned_allocs - before.pinned_allocs;
    g_setup_counts[2] = after.h2d_copies - before.h2d_copies;
    return made;
}

static void destroy_group(hprlp_solver **h, int count) {
    const long before = alloc_counts().device_frees;
    for (int k = 0; k < count; ++k) {
        try {
            destroy_handle(h[k]);
        } catch (...) {
        }
        h[k] = nullptr;
    }
    g_setup_counts[7] = alloc_counts().device_frees - before;
}

static void keep_scale_counts(const SetupCounts &sc) {
    g_setup_counts[3] = sc.scale_launches;
    g_setup_counts[4] = sc.scale_waits;
    g_setup_counts[5] = sc.served;
    g_setup_counts[6] = sc.own;
}

extern "C" int hprlp_solver_create_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, hprlp_solver **out) {
    GUARD_BEGIN
    for (int i = 0; i < 3; ++i) g_setup_counts[i] = 0;
    if (!models) throw std::runtime_error("hprlp_solver_create_many: null model list");
    if (count <= 0) throw std::runtime_error("hprlp_solver_create_many: count must be positive");
    if (!out) throw std::runtime_error("hprlp_solver_create_many: null handle list");
    HPRLP_parameters dflt;
    return create_group(models, count, param ? param : &dflt, out, "hprlp_solver_create_many", true);
    GUARD_END(-1)
}

extern "C" int hprlp_solver_scale_many(hprlp_solver **h, int count) {
    GUARD_BEGIN
    keep_scale_counts(SetupCounts());
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_scale_many", false);
    SetupCounts sc;
    scale_many(s.data(), count, &sc);
    keep_scale_counts(sc);
    return 0;
    GUARD_END(-1)
}

extern "C" void hprlp_solver_destroy_many(hprlp_solver **h, int count) {
    g_setup_counts[7] = 0;
    if (!h || count <= 0) return;
    destroy_group(h, count);
}

extern "C" int hprlp_solver_power_iteration_many(hprlp_solver **h, int count, int max_iter, double tol, double *lambda_out, int *iters_out) {
    GUARD_BEGIN
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_power_iteration_many");
    if (!lambda_out) throw std::runtime_error("hprlp_solver_power_iteration_many: null lambda_out");
    power_iteration_many(s.data(), count, max_iter, tol, lambda_out, iters_out);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_iterate_many(hprlp_solver **h, int count, const int *normal, int then_check) {
    GUARD_BEGIN
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_iterate_many");
    iterate_many(s.data(), count, normal, then_check != 0);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_residuals_many(hprlp_solver **h, int count, const int *iter, const int *compute_gap, double *out) {
    GUARD_BEGIN
    // (the plain arguments first, so that a wrong call is refused whatever the handles are)
    if (!iter) throw std::runtime_error("hprlp_solver_residuals_many: null iter");
    if (!compute_gap) throw std::runtime_error("hprlp_solver_residuals_many: null compute_gap");
    if (!out) throw std::runtime_error("hprlp_solver_residuals_many: null out");
    for (int k = 0; k < count; ++k)
        if (iter[k] < 0) throw std::runtime_error("hprlp_solver_residuals_many: iter[" + std::to_string(k) + "] is negative");
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_residuals_many");
    residuals_many(s.data(), count, iter, compute_gap, out);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_restart_many(hprlp_solver **h, int count, const double *in, double *sigma_out) {
    GUARD_BEGIN
    if (!in) throw std::runtime_error("hprlp_solver_restart_many: null in");
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_restart_many");
    restart_many(s.data(), count, in, sigma_out);
    return 0;
    GUARD_END(-1)
}

// counts of the calling thread's last hprlp_solver_run_many / hprlp_solve_many (hprlp_last_run_many_counts)
static thread_local long g_many_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static void keep_many_counts(const GroupCounts &gc) {
    keep_counts(g_many_counts, {gc.rounds, gc.waits, gc.group_launches, gc.copies, gc.own, gc.served, gc.ray_served, gc.certs_served});
}

extern "C" int hprlp_last_run_many_counts(long out[8]) { return read_counts(g_many_counts, out); }

static void free_results_arrays(HPRLP_results *out, int count) {
    for (int k = 0; k < count; ++k) {
        std::free(out[k].x); std::free(out[k].y); std::free(out[k].z);
        out[k].x = out[k].y = out[k].z = nullptr;
    }
}

extern "C" int hprlp_solver_run_many(hprlp_solver **h, int count, HPRLP_results *out) {
    GUARD_BEGIN
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_run_many");
    if (!out) throw std::runtime_error("hprlp_solver_run_many: null results");
    for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
    keep_many_counts(GroupCounts());
    try {
        GroupCounts gc;
        run_many(s.data(), count, out, &gc);
        keep_many_counts(gc);
    } catch (...) {
        free_results_arrays(out, count);
        throw;
    }
    return 0;
    GUARD_END(-1)
}

// ---- group re-solve, group matrix values, group device re-solve (DESIGN.md "Many small LPs") ------------------------------------
// counts of the calling thread's last hprlp_solver_set_data_many / _resolve_many (hprlp_last_resolve_many_counts) and
// hprlp_solver_set_matrix_values_many (hprlp_last_values_many_counts); the device entries put theirs in the same blocks, and what
// only a device call has in g_device_counts (hprlp_last_many_device_counts), which many.cpp fills as the call proceeds
static thread_local long g_resolve_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static thread_local long g_values_counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static thread_local DeviceCounts g_device_counts;
static void keep_resolve_counts(const ResolveCounts &rc) {
    keep_counts(g_resolve_counts, {rc.h2d, rc.d2h, rc.waits, rc.launches, rc.memsets, rc.served, rc.own, rc.loop_own});
}
static void keep_values_counts(const ValuesCounts &vc) {
    keep_counts(g_values_counts, {vc.h2d, vc.d2h, vc.waits, vc.launches, vc.memsets, vc.served, vc.own, vc.maps});
}

extern "C" int hprlp_last_resolve_many_counts(long out[8]) { return read_counts(g_resolve_counts, out); }
extern "C" int hprlp_last_values_many_counts(long out[8]) { return read_counts(g_values_counts, out); }
extern "C" int hprlp_last_many_device_counts(long out[8]) {
    const DeviceCounts &d = g_device_counts;
    return read_counts({d.pointers, d.lookups, d.check_launches, d.flags, d.served, d.own, d.waits_before_write, 0}, out);
}

// (Each entry zeroes its count blocks where it always did -- before or after the argument checks: the accessors show it.)
extern "C" int hprlp_solver_set_data_many(hprlp_solver **h, int count, const hprlp_member_data *data) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_set_data_many";
    check_group_args(h, count, data, "data", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberData> d = private_members<MemberData>(data, count);
    keep_resolve_counts(ResolveCounts());
    ResolveCounts rc;
    set_data_many(s.data(), count, d.data(), &rc);
    keep_resolve_counts(rc);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_resolve_many(hprlp_solver **h, int count, const hprlp_member_start *start, HPRLP_results *out) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_resolve_many";
    check_group_args(h, count, out, "results", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberStart> b = private_members<MemberStart>(start, count);
    check_starts(s.data(), count, b.data(), who, true);  // (before the results are touched: a refusal leaves the output arrays as they were)
    for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
    keep_resolve_counts(ResolveCounts());
    try {
        ResolveCounts rc;
        resolve_many(s.data(), count, b.data(), out, &rc);
        keep_resolve_counts(rc);
    } catch (...) {
        free_results_arrays(out, count);
        throw;
    }
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_matrix_values_many(hprlp_solver **h, int count, const hprlp_member_values *data) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_set_matrix_values_many";
    keep_values_counts(ValuesCounts());
    check_group_args(h, count, data, "data", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberValues> d = private_members<MemberValues>(data, count);
    ValuesCounts vc;
    set_matrix_values_many(s.data(), count, d.data(), &vc);
    keep_values_counts(vc);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_data_many_device(hprlp_solver **h, int count, const hprlp_member_data *data, void *stream) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_set_data_many_device";
    g_device_counts = DeviceCounts();
    keep_resolve_counts(ResolveCounts());
    check_group_args(h, count, data, "data", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberData> d = private_members<MemberData>(data, count);
    ResolveCounts rc;
    set_data_many_device(s.data(), count, d.data(), static_cast<hipStream_t>(stream), &rc, &g_device_counts);
    keep_resolve_counts(rc);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_resolve_many_device(hprlp_solver **h, int count, const hprlp_member_start *start, const hprlp_member_out *dst,
                                                void *stream, HPRLP_results *out) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_resolve_many_device";
    g_device_counts = DeviceCounts();
    keep_resolve_counts(ResolveCounts());
    check_group_args(h, count, out, "results", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberStart> b = private_members<MemberStart>(start, count);
    const std::vector<MemberOut> o = private_members<MemberOut>(dst, count);
    check_starts(s.data(), count, b.data(), who, false);  // (the starts' entries are the device check's)
    // (a refusal leaves the output array as it was: the results are touched once the call goes through)
    std::vector<HPRLP_results> res(static_cast<size_t>(count), make_error_result("ERROR"));
    ResolveCounts rc;
    resolve_many_device(s.data(), count, b.data(), o.data(), static_cast<hipStream_t>(stream), res.data(), &rc, &g_device_counts);
    keep_resolve_counts(rc);
    for (int k = 0; k < count; ++k) out[k] = res[k];  // (x, y, z are NULL: nothing for hprlp_free_results to free)
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_matrix_values_many_device(hprlp_solver **h, int count, const hprlp_member_values *data, void *stream) {
    GUARD_BEGIN
    const char *who = "hprlp_solver_set_matrix_values_many_device";
    g_device_counts = DeviceCounts();
    keep_values_counts(ValuesCounts());
    check_group_args(h, count, data, "data", who);
    std::vector<Solver *> s = group_members(h, count, who);
    const std::vector<MemberValues> d = private_members<MemberValues>(data, count);
    ValuesCounts vc;
    set_matrix_values_many_device(s.data(), count, d.data(), static_cast<hipStream_t>(stream), &vc, &g_device_counts);
    keep_values_counts(vc);
    return 0;
    GUARD_END(-1)
}

// phases of the calling thread's last hprlp_solve_many (hprlp_last_solve_many_phases)
static thread_local double g_many_phases[8] = {0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hprlp_last_solve_many_phases(double out[8]) {
    if (!out) return -1;
    for (int i = 0; i < 8; ++i) out[i] = g_many_phases[i];
    return 0;
}

// hprlp_solve_many, hprlp_solve_many_detect and hprlp_solve_many_wide (`who`, for the error messages; wide: every member is marked
// wide before the group's scaling).  det null: no detection.  certs (may be null):
// count entries, each cleared to its member's m and n on entry (hprlp_solve_detect's contract) and filled where detection ran.
static int solve_many_entry(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                            HPRLP_results *out, hprlp_certificate *certs, const char *who_, bool wide = false) {
    GUARD_BEGIN
    const std::string w(who_);
    if (!models) throw std::runtime_error(w + ": null model list");
    if (count <= 0) throw std::runtime_error(w + ": count must be positive");
    if (!out) throw std::runtime_error(w + ": null results");
    for (int k = 0; k < count; ++k)
        if (!models[k]) throw std::runtime_error(w + ": model " + std::to_string(k) + " is null");
    Detection dsel;
    bool with_det = false;
    try {
        with_det = detection_from(det, &dsel);  // (a negative eps: refused before anything is created)
    } catch (const std::exception &e) {
        throw std::runtime_error(w + ": " + e.what());
    }
    if (certs)
        for (int k = 0; k < count; ++k) clear_certificate(&certs[k], models[k]->m, models[k]->n);
    HPRLP_parameters dflt;
    const HPRLP_parameters *p = param ? param : &dflt;
    const auto t_call = time_now();
    for (int k = 0; k < count; ++k) out[k] = make_error_result("ERROR");
    for (int i = 0; i < 8; ++i) g_many_phases[i] = 0.0;
    keep_many_counts(GroupCounts());
    for (int i = 0; i < 8; ++i) g_setup_counts[i] = 0;
    // set-up and scaling of the whole group (create_group, scale_many); a model that fails its set-up stays "ERROR" and the others
    // go on.  HPRLP_NO_GROUP_SETUP=1 (test hook, A/B runs): member by member, as hprlp_solver_create + hprlp_solver_scale.
    const char *ngs = env_get("HPRLP_NO_GROUP_SETUP");
    const bool together = !(ngs && ngs[0] == '1');
    std::vector<hprlp_solver *> owned(static_cast<size_t>(count), nullptr);
    struct Teardown {  // (the members' device state goes when the call ends, however it ends)
        std::vector<hprlp_solver *> &h;
        ~Teardown() {
            for (hprlp_solver *m : h)
                if (m) {
                    destroy_group(h.data(), static_cast<int>(h.size()));
                    return;
                }
        }
    } teardown{owned};
    std::vector<Solver *> s;
    std::vector<int> who;
    const auto t_setup = time_now();
    create_group(models, count, p, owned.data(), who_, together);
    g_many_phases[0] = time_since(t_setup);
    for (int k = 0; k < count; ++k)
        if (owned[k]) {
            owned[k]->s.group_wide = wide;  // (hprlp_solve_many_wide: every member asks for the group launches)
            s.push_back(&owned[k]->s);
            who.push_back(k);
        }
    const int ng = static_cast<int>(s.size());
    if (ng > 0) {
        const auto t_scale = time_now();
        SetupCounts sc;
        if (together) {
            scale_many(s.data(), ng, &sc);
        } else {
            const long l0 = scaling_launch_count();
            for (int g = 0; g < ng; ++g) {
                const long f0 = s[g]->fetches;
                s[g]->scale();
                sc.scale_waits += s[g]->fetches - f0 + 1;
                ++sc.own;
            }
            sc.scale_launches = scaling_launch_count() - l0;
        }
        keep_scale_counts(sc);
        g_many_phases[1] = time_since(t_scale);
        std::vector<HPRLP_results> res(static_cast<size_t>(ng));
        for (auto &r : res) r = make_error_result("ERROR");
        try {
            const auto t_pw = time_now();
            std::vector<double> lam(static_cast<size_t>(ng));
            power_iteration_many(s.data(), ng, 5000, 1e-4, lam.data(), nullptr);  // src/HPRLP.cu:81-97
            for (int g = 0; g < ng; ++g) {
                s[g]->lambda_max = lam[g] * 1.01;
                s[g]->init_iteration_state();
                if (with_det) s[g]->detect = dsel;
            }
            g_many_phases[2] = time_since(t_pw);
            const WideCounts pw = last_wide_counts();
            const auto t_loop = time_now();
            GroupCounts gc;
            run_many(s.data(), ng, res.data(), &gc);
            if (wide) last_wide_counts().power_launches = pw.power_launches, last_wide_counts().power_waits = pw.power_waits;
            g_many_phases[3] = time_since(t_loop);  // (the loop and the solutions' way back)
            g_many_phases[5] = static_cast<double>(gc.rounds);
            g_many_phases[6] = static_cast<double>(gc.waits);
            g_many_phases[7] = static_cast<double>(gc.launches);
            keep_many_counts(gc);
            if (with_det && certs)
                for (int g = 0; g < ng; ++g)
                    if (!export_certificate(s[g]->cert, &certs[who[g]], models[who[g]]->m, models[who[g]]->n)) {
                        for (int k = 0; k < count; ++k) hprlp_free_certificate(&certs[k]);
                        throw std::runtime_error(w + ": host allocation of a certificate failed");
                    }
        } catch (...) {
            free_results_arrays(res.data(), ng);
            throw;
        }
        for (int g = 0; g < ng; ++g) out[who[g]] = res[g];
    }
    destroy_group(owned.data(), count);  // (the members' device state goes here: part of the call's wall time)
    g_many_phases[4] = time_since(t_call);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solve_many(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, HPRLP_results *out) {
    return solve_many_entry(models, count, param, nullptr, out, nullptr, "hprlp_solve_many");
}

extern "C" int hprlp_solve_many_detect(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                                       HPRLP_results *out, hprlp_certificate *certs) {
    return solve_many_entry(models, count, param, det, out, certs, "hprlp_solve_many_detect");
}

// ---- wide members (many.cpp; DESIGN.md "Many small LPs", wide members) -------------------------------------------------------
extern "C" int hprlp_solver_set_group_wide(hprlp_solver *h, int on) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("hprlp_solver_set_group_wide: null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_group_wide: a sharded solver (hprlp_solver_create_dist* / _local*) joins no group; a group runs on one GPU");
    h->s.group_wide = on != 0;
    if (h->s.use_small && !h->s.comm) return 1;  // (it joins anyway)
    return on != 0 && h->s.joins_group() ? 1 : 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solve_many_wide(const LP_info_cpu *const *models, int count, const HPRLP_parameters *param, const hprlp_detection *det,
                                     HPRLP_results *out, hprlp_certificate *certs) {
    return solve_many_entry(models, count, param, det, out, certs, "hprlp_solve_many_wide", true);
}

extern "C" int hprlp_last_many_wide_counts(long out[8]) {
    if (!out) return -1;
    const WideCounts &wc = last_wide_counts();
    const long v[8] = {wc.joined, wc.refused, wc.normal_launches, wc.segments, wc.member_iterations, wc.power_launches, wc.power_waits, 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 0;
}

namespace {
struct VecRef {
    double *p;
    long n;
    char kind;  // 'r': per row of A, 'c': per column, '-': raw (matrix values)
};
VecRef find_vector(Solver &s, const std::string &name) {
    if (name == "x") return {s.x.p, s.n_loc, 'c'};
    if (name == "last_x") return {s.last_x.p, s.n_loc, 'c'};
    if (name == "x_hat") return {s.x_hat, s.n_loc, 'c'};
    if (name == "x_bar") return {s.x_bar, s.n_loc, 'c'};
    if (name == "z_bar") return {s.z_bar.p, s.n_loc, 'c'};
    if (name == "x_temp") return {s.x_temp, s.n_loc, 'c'};
    if (name == "y") return {s.y, s.m_loc, 'r'};
    if (name == "last_y") return {s.last_y.p, s.m_loc, 'r'};
    if (name == "y_bar") return {s.y_bar, s.m_loc, 'r'};
    if (name == "y_obj") return {s.y_obj.p, s.m_loc, 'r'};
    if (name == "y_temp") return {s.y_temp.p, s.m_loc, 'r'};
    if (name == "AL") return {s.AL.p, s.m_loc, 'r'};
    if (name == "AU") return {s.AU.p, s.m_loc, 'r'};
    if (name == "l") return {s.l.p, s.n_loc, 'c'};
    if (name == "u") return {s.u.p, s.n_loc, 'c'};
    if (name == "c") return {s.c.p, s.n_loc, 'c'};
    if (name == "row_norm") return {s.row_norm.p, s.m_loc, 'r'};
    if (name == "col_norm") return {s.col_norm.p, s.n_loc, 'c'};
    if (name == "A_val") return {s.A.val.p, s.A.view.nnz, '-'};
    if (name == "AT_val") return {s.AT.val.p, s.AT.view.nnz, '-'};
    // the power iteration's two scratch vectors (the scaling's gathered ones), this rank's slices: zero between the phases
    if (name == "gsm") return {s.gsm.p + s.row_off, s.m_loc, 'r'};
    if (name == "gsn") return {s.gsn.p + s.col_off, s.n_loc, 'c'};
    if (s.ray_prev_x.p) {  // the ray test's vectors, once Solver::ray_begin has allocated them (scaled units)
        if (name == "ray_d") return {s.ray_d.p, s.n_loc, 'c'};
        if (name == "ray_prev_x") return {s.ray_prev_x.p, s.n_loc, 'c'};
        if (name == "ray_y") return {s.ray_y.p, s.m_loc, 'r'};
        if (name == "ray_prev_y") return {s.ray_prev_y.p, s.m_loc, 'r'};
    }
    return {nullptr, -1, '-'};
}
// the permutation (device index -> caller's index) that applies to a vector, or null
const std::vector<int> *perm_of(const Solver &s, const VecRef &v) {
    if (v.kind == 'r' && !s.perm_r.empty()) return &s.perm_r;
    if (v.kind == 'c' && !s.perm_c.empty()) return &s.perm_c;
    return nullptr;
}
}  // namespace

// Vectors travel in the caller's numbering: with a set-up time locality ordering in place (solver.h: perm_r / perm_c)
// the device order is un-permuted on the way out and permuted on the way in.  A_val / AT_val are the device arrays as
// they are (entries of the permuted matrix).
extern "C" long hprlp_solver_get_vector(hprlp_solver *h, const char *name, double *out, long cap) {
    GUARD_BEGIN
    VecRef v = find_vector(h->s, name ? name : "");
    if (v.n < 0) throw std::runtime_error(std::string("unknown vector name: ") + (name ? name : "(null)"));
    if (cap < v.n) throw std::runtime_error("output buffer too small");
    HIP_CHECK(hipStreamSynchronize(h->s.stream));
    if (v.n > 0) {
        if (const std::vector<int> *perm = perm_of(h->s, v)) {
            std::vector<double> tmp(static_cast<size_t>(v.n));
            HIP_CHECK(hipMemcpy(tmp.data(), v.p, sizeof(double) * v.n, hipMemcpyDeviceToHost));
            for (long i = 0; i < v.n; ++i) out[(*perm)[i]] = tmp[i];
        } else {
            HIP_CHECK(hipMemcpy(out, v.p, sizeof(double) * v.n, hipMemcpyDeviceToHost));
        }
    }
    return v.n;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_vector(hprlp_solver *h, const char *name, const double *in, long len) {
    GUARD_BEGIN
    VecRef v = find_vector(h->s, name ? name : "");
    if (v.n < 0) throw std::runtime_error(std::string("unknown vector name: ") + (name ? name : "(null)"));
    if (len != v.n) throw std::runtime_error("length mismatch");
    h->s.invalidate_far();
    HIP_CHECK(hipStreamSynchronize(h->s.stream));
    if (v.n > 0) {
        if (const std::vector<int> *perm = perm_of(h->s, v)) {
            std::vector<double> tmp(static_cast<size_t>(v.n));
            for (long i = 0; i < v.n; ++i) tmp[i] = in[(*perm)[i]];
            HIP_CHECK(hipMemcpy(v.p, tmp.data(), sizeof(double) * v.n, hipMemcpyHostToDevice));
        } else {
            HIP_CHECK(hipMemcpy(v.p, in, sizeof(double) * v.n, hipMemcpyHostToDevice));
        }
    }
    if (v.p == h->s.l.p || v.p == h->s.u.p || v.p == h->s.AL.p || v.p == h->s.AU.p) {  // the bound codes follow the arrays
        h->s.refresh_bound_codes();
        HIP_CHECK(hipStreamSynchronize(h->s.stream));
    }
    return 0;
    GUARD_END(-1)
}

// Locality ordering of a CSR pattern (reorder.cpp), host only: out = {accepted (0/1), tiled share of the entries before,
// after, clusters, components, seconds}; the permutations (new -> old) are written only when accepted.
extern "C" int hprlp_locality_ordering(int m, int n, const int *rowptr, const int *col, int *row_new2old, int *col_new2old, double out[6]) {
    try {
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
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
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
    try {
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
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_permute_csr_device(int m, int n, const int *rowptr, const int *col, const double *val, const int *row_new2old,
                                        const int *col_new2old, int *rp_out, int *ci_out, double *val_out) {
    try {
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
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_tiling_share(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                                  int on_device, double *share) {
    try {
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
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: the stream kernel's row blocks of a CSR pattern (split rows, chunks by column eighths), built and checked as a
// solver's set-up does.  out = {blocks, split rows, chunk slots, rows cut by column eighths, longest chunk, entries covered}.
extern "C" int hprlp_row_block_plan(int m, int n, const int *rowptr, const int *col, int with_cuts, long out[6]) {
    try {
        if (m <= 0 || n <= 0 || !rowptr || !col || !out) throw std::runtime_error("bad arguments");
        row_block_plan_host(m, n, rowptr, col, with_cuts != 0, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// Host only: what solve_batched does to a batch's vectors before anything is uploaded (batch_prep.h), on plain arrays
extern "C" int hprlp_batched_prepare_host(int m, int n, int B, const double *rn, const double *cn, const double *C, const double *AL,
                                          const double *AU, const double *l, const double *u, const double *X0, const double *Y0,
                                          int use_bc_scaling, hprlp_batched_prepared *out) {
    return hprlp_batched_prepare_host_rule(m, n, B, rn, cn, C, AL, AU, l, u, X0, Y0, use_bc_scaling, kNormRuleReference, out);
}

extern "C" int hprlp_batched_prepare_host_rule(int m, int n, int B, const double *rn, const double *cn, const double *C,
                                               const double *AL, const double *AU, const double *l, const double *u, const double *X0,
                                               const double *Y0, int use_bc_scaling, int norm_rule, hprlp_batched_prepared *out) {
    try {
        if (m <= 0 || n <= 0 || B <= 0 || !rn || !cn || !C || !AL || !AU || !l || !u || !out) throw std::runtime_error("bad arguments");
        const BatchData d = prepare_batch(m, n, B, C, AL, AU, l, u, nullptr, 0.0, rn, cn, use_bc_scaling != 0, norm_rule);
        const size_t nB = static_cast<size_t>(n) * B, mB = static_cast<size_t>(m) * B;
        auto give = [](const std::vector<double> &v, double *dst) {
            if (dst) std::copy(v.begin(), v.end(), dst);
        };
        give(d.C, out->C); give(d.AL, out->AL); give(d.AU, out->AU); give(d.L, out->l); give(d.U, out->u);
        const std::vector<double> *scalars[7] = {&d.b_scale, &d.c_scale, &d.norm_b, &d.norm_c, &d.norm_b_org, &d.norm_c_org, &d.sigma};
        for (int i = 0; i < 7 && out->scalars; ++i) give(*scalars[i], out->scalars + static_cast<size_t>(i) * B);
        // a start into scaled units, and from there back as a solution goes
        auto there_and_back = [B](const double *v0, size_t len, int rows, const double *norm, const std::vector<double> &scale,
                                  double *scaled, double *back) {
            if (!v0) return;
            std::vector<double> v(v0, v0 + len);
            start_to_scaled(v.data(), rows, B, norm, scale);
            if (scaled) std::copy(v.begin(), v.end(), scaled);
            point_to_caller(v.data(), rows, B, norm, scale);
            if (back) std::copy(v.begin(), v.end(), back);
        };
        there_and_back(X0, nB, n, cn, d.b_scale, out->X0, out->X_back);
        there_and_back(Y0, mB, m, rn, d.c_scale, out->Y0, out->Y_back);
        if (out->z_back) {  // z = (Z * cn) * c_scale of the scaled C
            give(d.C, out->z_back);
            reduced_cost_to_caller(out->z_back, n, B, cn, d.c_scale);
        }
        out->Bp = padded_batch(B);
        out->Bc = choose_chunk(m, n, out->Bp);
        const Geo geo = make_geo(out->Bp, out->Bc);
        std::vector<double> panel;
        to_panel(d.C, n, B, geo, out->pad, panel);
        give(panel, out->panel);
        if (out->panel_back) from_panel(panel, n, B, geo, out->panel_back);
        for (int k = 0; k < B && out->panel_index; ++k)
            for (int i = 0; i < n; ++i) out->panel_index[static_cast<size_t>(k) * n + i] = static_cast<long>(panel_index(geo, n, i, k));
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_solver_get_scalars(hprlp_solver *h, double out[16]) {
    GUARD_BEGIN
    Solver &s = h->s;
    Ctrl ck;
    HIP_CHECK(hipStreamSynchronize(s.stream));
    HIP_CHECK(hipMemcpy(&ck, s.ctrl.p, sizeof(Ctrl), hipMemcpyDeviceToHost));
    const double v[16] = {s.b_scale, s.c_scale, s.norm_b, s.norm_c, s.norm_b_org, s.norm_c_org, s.sigma, s.lambda_max,
                          s.setup_time, s.scaling_time, s.power_time, static_cast<double>(s.power_iters),
                          static_cast<double>(ck.kx), static_cast<double>(ck.ky), 0, 0};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_info(hprlp_solver *h, long out[8]) {
    GUARD_BEGIN
    Solver &s = h->s;
    s.finish_tiling();  // report the kernels that will actually run
    out[0] = s.m; out[1] = s.n; out[2] = s.A.view.nnz;
    out[3] = s.A.view.nblk; out[4] = s.AT.view.nblk;
    out[5] = s.A.view.grid(); out[6] = s.AT.view.grid();
    // bit0: A tiled, bit1: A^T tiled, bit2: normal iterations run in the single-workgroup small-LP kernel
    // bit3: a set-up time locality ordering is in place (the device works on P A Q)
    out[7] = (s.A.view.tiled.valid ? 1 : 0) + (s.AT.view.tiled.valid ? 2 : 0) + (s.use_small && !s.comm ? 4 : 0) + (s.perm_r.empty() ? 0 : 8);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_detection(hprlp_solver *h, const hprlp_detection *det) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("null solver");
    if (h->sharded && det)
        throw std::runtime_error("hprlp_solver_set_detection: infeasibility detection runs on one GPU only; a sharded solver "
                                 "(hprlp_solver_create_dist* / _local*) refuses it");
    Detection d;
    detection_from(det, &d);
    h->s.detect = d;
    return 0;
    GUARD_END(-1)
}

// One ray test outside the loop: the evaluation a periodic check of solve_loop runs (residuals with the gap, then the ray test,
// one fetch), so the nine slots come the way the loop reads them.  Solver::detect is not touched.
extern "C" int hprlp_solver_ray_step(hprlp_solver *h, int restart, double out[9]) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("null solver / output");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_ray_step: infeasibility detection runs on one GPU only; a sharded solver "
                                 "(hprlp_solver_create_dist* / _local*) refuses it");
    Solver &s = h->s;
    if (restart) s.ray_begin();
    else if (!s.ray_prev_x.p) throw std::runtime_error("hprlp_solver_ray_step: the first step of a solver needs restart != 0");
    Residuals r;
    RestartState rs;
    bool ray = false;
    s.compute_residuals(1, true, &r, &rs, &ray);
    if (!ray) return 0;
    const int slots[9] = {S_RAY_DY, S_RAY_CD, S_RAY_VY, S_RAY_WD, S_RAY_YN, S_RAY_DN, S_RAY_DZ, S_RAY_VZ, S_RAY_WQ};
    for (int k = 0; k < 9; ++k) out[k] = s.scal_h[slots[k]];
    return 1;
    GUARD_END(-1)
}

// hprlp_solver_ray_step for every member of a group (many.cpp: ray_step_many)
extern "C" int hprlp_solver_ray_step_many(hprlp_solver **h, int count, const int *restart, double *out, int *tested) {
    GUARD_BEGIN
    // (the plain arguments first, so that a wrong call is refused whatever the handles are)
    if (!restart) throw std::runtime_error("hprlp_solver_ray_step_many: null restart");
    if (!out) throw std::runtime_error("hprlp_solver_ray_step_many: null out");
    if (!tested) throw std::runtime_error("hprlp_solver_ray_step_many: null tested");
    std::vector<Solver *> s = group_members(h, count, "hprlp_solver_ray_step_many");
    ray_step_many(s.data(), count, restart, out, tested);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_start(hprlp_solver *h, const double *x0, const double *y0) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_start: warm start runs on one GPU only; a sharded solver (hprlp_solver_create_dist* / "
                                 "_local*) refuses it");
    check_start(x0, h->s.n, "x0");
    check_start(y0, h->s.m, "y0");
    h->s.set_start(x0, y0);
    return 0;
    GUARD_END(-1)
}

// Re-solve (DESIGN.md "Re-solve"): new data for the resident LP, then a further solve on the same solver
extern "C" int hprlp_solver_set_data(hprlp_solver *h, const double *c, const double *obj_constant, const double *AL, const double *AU,
                                     const double *l, const double *u) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_data: new data for a resident model runs on one GPU only; a sharded solver "
                                 "(hprlp_solver_create_dist* / _local*) refuses it");
    h->s.set_data(c, obj_constant, AL, AU, l, u);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_resolve(hprlp_solver *h, double sigma, const double *x0, const double *y0, HPRLP_results *out,
                                    hprlp_trace_row *trace, int max_trace, int *n_trace) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("null solver / result");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_resolve: a re-solve runs on one GPU only; a sharded solver (hprlp_solver_create_dist* / "
                                 "_local*) refuses it");
    if (std::isnan(sigma)) throw std::runtime_error("hprlp_solver_resolve: sigma is NaN");
    check_start(x0, h->s.n, "x0");
    check_start(y0, h->s.m, "y0");
    Solver &s = h->s;
    s.trace = reinterpret_cast<TraceRow *>(trace);
    s.trace_cap = trace ? max_trace : 0;
    try {
        s.resolve(sigma, x0, y0, out);
    } catch (...) {
        s.trace = nullptr;
        s.trace_cap = 0;
        throw;
    }
    if (n_trace) *n_trace = s.trace_n;
    s.trace = nullptr;
    s.trace_cap = 0;
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_data_seconds(hprlp_solver *h, double out[3]) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("null solver / output");
    for (int i = 0; i < 3; ++i) out[i] = h->s.data_time[i];
    return 0;
    GUARD_END(-1)
}

// Matrix values (DESIGN.md "Matrix values"): new values on the resident pattern, then hprlp_solver_power_iteration / _init / _resolve
extern "C" int hprlp_solver_set_matrix_values(hprlp_solver *h, const double *val, long nnz, const double *c, const double *obj_constant,
                                              const double *AL, const double *AU, const double *l, const double *u) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("hprlp_solver_set_matrix_values: null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_matrix_values: new matrix values for a resident model run on one GPU only; a sharded "
                                 "solver (hprlp_solver_create_dist* / _local*) refuses them");
    h->s.set_matrix_values(val, nnz, c, obj_constant, AL, AU, l, u);
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_matrix_seconds(hprlp_solver *h, double out[6]) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("hprlp_solver_matrix_seconds: null solver / output");
    for (int i = 0; i < 5; ++i) out[i] = h->s.matrix_time[i];
    out[5] = static_cast<double>(h->s.matrix_calls);
    return 0;
    GUARD_END(-1)
}

// Device-resident re-solve (DESIGN.md "Device-resident re-solve"): the three entries above with the vectors in device memory
extern "C" int hprlp_solver_set_data_device(hprlp_solver *h, const double *dc, const double *obj_constant, const double *dAL,
                                            const double *dAU, const double *dl, const double *du, void *stream) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("hprlp_solver_set_data_device: null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_data_device: new data for a resident model runs on one GPU only; a sharded solver "
                                 "(hprlp_solver_create_dist* / _local*) refuses it");
    h->s.set_data_device(dc, obj_constant, dAL, dAU, dl, du, static_cast<hipStream_t>(stream));
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_resolve_device(hprlp_solver *h, double sigma, const double *dx0, const double *dy0, void *stream, double *dx,
                                           double *dy, double *dz, HPRLP_results *out, hprlp_trace_row *trace, int max_trace,
                                           int *n_trace) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("hprlp_solver_resolve_device: null solver / result");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_resolve_device: a re-solve runs on one GPU only; a sharded solver (hprlp_solver_create_dist* / "
                                 "_local*) refuses it");
    if (std::isnan(sigma)) throw std::runtime_error("hprlp_solver_resolve_device: sigma is NaN");
    Solver &s = h->s;
    s.trace = reinterpret_cast<TraceRow *>(trace);
    s.trace_cap = trace ? max_trace : 0;
    try {
        s.resolve_device(sigma, dx0, dy0, static_cast<hipStream_t>(stream), dx, dy, dz, out);
    } catch (...) {
        s.trace = nullptr;
        s.trace_cap = 0;
        throw;
    }
    if (n_trace) *n_trace = s.trace_n;
    s.trace = nullptr;
    s.trace_cap = 0;
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_set_matrix_values_device(hprlp_solver *h, const double *dval, long nnz, const double *dc,
                                                     const double *obj_constant, const double *dAL, const double *dAU, const double *dl,
                                                     const double *du, void *stream) {
    GUARD_BEGIN
    if (!h) throw std::runtime_error("hprlp_solver_set_matrix_values_device: null solver");
    if (h->sharded)
        throw std::runtime_error("hprlp_solver_set_matrix_values_device: new matrix values for a resident model run on one GPU only; a "
                                 "sharded solver (hprlp_solver_create_dist* / _local*) refuses them");
    h->s.set_matrix_values_device(dval, nnz, dc, obj_constant, dAL, dAU, dl, du, static_cast<hipStream_t>(stream));
    return 0;
    GUARD_END(-1)
}

extern "C" int hprlp_solver_transfer(hprlp_solver *h, long out[4]) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("hprlp_solver_transfer: null solver / output");
    for (int i = 0; i < 4; ++i) out[i] = h->s.transfer[i];
    return 0;
    GUARD_END(-1)
}

// The value maps as the solver built them (built here if no hprlp_solver_set_matrix_values call has done it yet); mapA / mapAT
// receive nnz ints each.  Returns nnz.
extern "C" long hprlp_solver_value_maps(hprlp_solver *h, int *mapA, int *mapAT, long cap) {
    GUARD_BEGIN
    if (!h || !mapA || !mapAT) throw std::runtime_error("hprlp_solver_value_maps: null solver / output");
    if (h->sharded) throw std::runtime_error("hprlp_solver_value_maps: one GPU only; a sharded solver has no value maps");
    Solver &s = h->s;
    const long nnz = s.A.view.nnz;
    if (cap < nnz) throw std::runtime_error("hprlp_solver_value_maps: output buffers too small");
    s.build_value_maps();
    HIP_CHECK(hipStreamSynchronize(s.stream));
    if (nnz > 0) {
        if (s.map_A.p) HIP_CHECK(hipMemcpy(mapA, s.map_A.p, sizeof(int) * nnz, hipMemcpyDeviceToHost));
        else
            for (long e = 0; e < nnz; ++e) mapA[e] = static_cast<int>(e);
        HIP_CHECK(hipMemcpy(mapAT, s.map_AT.p, sizeof(int) * nnz, hipMemcpyDeviceToHost));
    }
    return nnz;
    GUARD_END(-1)
}

// Host only: the rule of the value maps restated (values_host.cpp); row_new2old / col_new2old null: no ordering
extern "C" int hprlp_value_maps_host(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old,
                                     int *mapA, int *mapAT) {
    try {
        value_maps_host(m, n, rowptr, col, row_new2old, col_new2old, mapA, mapAT);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

// The locality ordering a solver applied: row_new2old (m) / col_new2old (n) as perm_r / perm_c hold them.  Returns 1 with the
// arrays filled, 0 without an ordering (arrays untouched).
extern "C" int hprlp_solver_ordering(hprlp_solver *h, int *row_new2old, int *col_new2old) {
    GUARD_BEGIN
    if (!h || !row_new2old || !col_new2old) throw std::runtime_error("hprlp_solver_ordering: null solver / output");
    const Solver &s = h->s;
    if (s.perm_r.empty()) return 0;
    std::copy(s.perm_r.begin(), s.perm_r.end(), row_new2old);
    std::copy(s.perm_c.begin(), s.perm_c.end(), col_new2old);
    return 1;
    GUARD_END(-1)
}

// The power iteration's start vector as Solver::power_start leaves it on the device, in the caller's numbering.
extern "C" int hprlp_solver_power_start(hprlp_solver *h, double *out, int cap) {
    GUARD_BEGIN
    if (!h || !out) throw std::runtime_error("hprlp_solver_power_start: null solver / output");
    Solver &s = h->s;
    if (s.comm) throw std::runtime_error("hprlp_solver_power_start: single-GPU solvers only");
    if (cap < s.m_loc) throw std::runtime_error("hprlp_solver_power_start: output too short");
    s.power_start(s.sm1.p);
    std::vector<double> z(static_cast<size_t>(std::max(s.m_loc, 1)));
    HIP_CHECK(hipMemcpy(z.data(), s.sm1.p, sizeof(double) * static_cast<size_t>(s.m_loc), hipMemcpyDeviceToHost));
    for (int i = 0; i < s.m_loc; ++i) out[s.perm_r.empty() ? i : s.perm_r[i]] = z[i];
    return s.m_loc;
    GUARD_END(-1)
}

extern "C" int hprlp_batched_solver_set_matrix_values(hprlp_batched_solver *h, const double *val, long nnz) {
    try {
        if (!h || !h->s) throw std::runtime_error("hprlp_batched_solver_set_matrix_values: null solver");
        batched_solver_set_matrix_values(h->s, val, nnz);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_solver_get_certificate(hprlp_solver *h, hprlp_certificate *cert) {
    GUARD_BEGIN
    if (!h || !cert) throw std::runtime_error("null solver / certificate");
    if (!export_certificate(h->s.cert, cert, h->s.m, h->s.n)) throw std::runtime_error("host allocation of the certificate failed");
    return 0;
    GUARD_END(-1)
}

// One line per matrix saying which kernel form runs and on what structure (bench.py's ladder, tools/run_mps_dir.py)
extern "C" int hprlp_solver_describe(hprlp_solver *h, char *buf, int cap) {
    GUARD_BEGIN
    if (!h || !buf || cap <= 0) throw std::runtime_error("null solver / buffer");
    Solver &s = h->s;
    s.finish_tiling();
    auto one = [](const char *name, const DeviceMatrix &M) {
        const TiledDev &t = M.view.tiled;
        std::string d = std::string(name) + ": ";
        if (!t.valid) {
            d += "stream kernel (k_spmv_fused, " + std::to_string(M.view.nblk) + " row blocks, " + std::to_string(M.view.nlong) + " split rows)";
            d += no_tiled_note(M.outcome.why);
            return d;
        }
        d += t.n_pieces > 0 ? "tiled, piece form (k_tiled_part + k_tiled_finish, " + std::to_string(t.n_pieces) + " pieces)"
             : t.rem_cap == kPbRemCap ? "tiled, all-remainder form (k_pb_fused, grid " + std::to_string(t.grid) + ")"
                                      : "tiled, fused (k_tiled_fused, grid " + std::to_string(t.grid) + ")";
        d += ", " + std::to_string(t.nsb) + " super-blocks, " + std::to_string(M.tiled.n_steps) + " steps";
        if (t.R != kTileRows || t.T != kTileCols) d += " (" + std::to_string(t.R) + " rows, tiles of " + std::to_string(t.T) + " columns)";
        const double all = static_cast<double>(M.tiled.dense_entries) + static_cast<double>(M.tiled.n_rem);
        if (all > 0) d += ", " + std::to_string(static_cast<int>(100.0 * M.tiled.dense_entries / all + 0.5)) + " % of the entries in staged tiles";
        if (t.f_rk) d += ", source-side run tables";
        if (t.f_work) d += ", pre-pass work list of " + std::to_string(t.n_work) + " workgroups for " + std::to_string(t.n_groups) + " source groups";
        if (t.side_nblk > 0) d += ", long rows aside (" + std::to_string(t.side_nblk) + " blocks through the stream kernel)";
        if (t.repeats) d += ", repeats";  // (some tile has several steps: the <.., REP = true> instantiations run)
        return d;
    };
    std::string d = one("A", s.A) + "; " + one("A^T", s.AT);
    if (s.use_small && !s.comm) d += "; normal iterations in the single-workgroup kernel (k_small_iterations)";
    if (!s.perm_r.empty()) d += "; locality ordering applied at set-up";
    // (anything but the default path says so: the switches this solver was set up under, and hooks that were set but not honoured)
    if (!s.env_at_setup.empty()) d += "; switches: " + s.env_at_setup;
    if (!s.env_ignored_at_setup.empty()) d += "; ignored without HPRLP_TEST_HOOKS=1: " + s.env_ignored_at_setup;
    std::snprintf(buf, static_cast<size_t>(cap), "%s", d.c_str());
    return static_cast<int>(d.size());
    GUARD_END(-1)
}

// Host only: the staged decisions of the kernel-form selection (form_select.h) for a facts record
extern "C" int hprlp_form_select(const hprlp_form_facts *facts, const hprlp_form_hooks *hooks, hprlp_form_decision *out) {
    try {
        if (!facts || !out) throw std::runtime_error("bad arguments");
        const char *missing = "";
        if (!form_select(*facts, hooks ? *hooks : FormHooks(), out, &missing))
            throw std::runtime_error(std::string("the rules ask for a fact that the record marks as not measured: ") + missing);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
}

extern "C" int hprlp_solver_form_facts(hprlp_solver *h, int which, hprlp_form_facts out[2]) {
    GUARD_BEGIN
    if (!h || !out || which < 0 || which > 1) throw std::runtime_error("null solver / buffer, or no such matrix");
    h->s.finish_tiling();
    const DeviceMatrix &M = which ? h->s.AT : h->s.A;
    out[0] = M.facts;
    out[1] = M.facts_pb;
    return M.passes;
    GUARD_END(-1)
}

// Host only: the column-tiled structure of a CSR pattern (host builder, tiled.cpp) with super-blocks of R rows and tiles of T
// columns, verified entry by entry (every entry once, codes name their entries, one chunk per accumulator inside a step, layers).
// out = {tile entries incl. padding, remainder entries, steps, padding, most consecutive steps of one tile, staged share x 1e6}.
extern "C" int hprlp_tiled_host_check(int m, int n, const int *rowptr, const int *col, int R, int T, double min_dense, long out[6]) {
    try {
        if (m <= 0 || n <= 0 || !rowptr || !col || !out) throw std::runtime_error("bad arguments");
        tiled_host_check(m, n, rowptr, col, R, T, min_dense, out);
        return 0;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return -1;
    }
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

extern "C" int hprlp_solver_time_iterations(hprlp_solver *h, int warmup, int steps, int mode, double *total_ms,
                                            double *xhalf_ms, double *yhalf_ms) {
    GUARD_BEGIN
    Solver &s = h->s;
    if (steps <= 0) throw std::runtime_error("steps must be positive");
    s.run_normal(warmup);
    HIP_CHECK(hipStreamSynchronize(s.stream));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    double tx = 0, ty = 0;
    float ms = 0;
    if (mode == 0) {
        HIP_CHECK(hipEventRecord(e0, s.stream));
        s.run_normal(steps);
        HIP_CHECK(hipEventRecord(e1, s.stream));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    } else if (mode == 2) {
        s.invalidate_far();
        // the bare SpMVs of the path (A^T y into scratch, A x_hat into scratch): no half-step update, no state change
        std::vector<hipEvent_t> ev(static_cast<size_t>(steps) * 3);
        for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
        HIP_CHECK(hipEventRecord(e0, s.stream));
        for (int i = 0; i < steps; ++i) {
            HIP_CHECK(hipEventRecord(ev[3 * i], s.stream));
            launch_spmv_plain(s.AT.view, s.gy.p, s.sn1.p, nullptr, false, nullptr, 0, s.stream);
            HIP_CHECK(hipEventRecord(ev[3 * i + 1], s.stream));
            launch_spmv_plain(s.A.view, s.gxh.p, s.sm1.p, nullptr, false, nullptr, 0, s.stream);
            HIP_CHECK(hipEventRecord(ev[3 * i + 2], s.stream));
        }
        HIP_CHECK(hipEventRecord(e1, s.stream));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        for (int i = 0; i < steps; ++i) {
            float a = 0, b = 0;
            HIP_CHECK(hipEventElapsedTime(&a, ev[3 * i], ev[3 * i + 1]));
            HIP_CHECK(hipEventElapsedTime(&b, ev[3 * i + 1], ev[3 * i + 2]));
            tx += a;
            ty += b;
        }
        for (auto &e : ev) (void)hipEventDestroy(e);
    } else {
        std::vector<hipEvent_t> ev(static_cast<size_t>(steps) * 3);
        for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
        // the solver's own normal pair (with the multi-GPU overlap when it is on): events before / between / after the halves
        HIP_CHECK(hipEventRecord(e0, s.stream));
        for (int i = 0; i < steps; ++i) s.launch_normal_pair(i + 1 < steps, &ev[3 * static_cast<size_t>(i)], s.x_mode_of(i, steps));
        HIP_CHECK(hipEventRecord(e1, s.stream));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        for (int i = 0; i < steps; ++i) {
            float a = 0, b = 0;
            HIP_CHECK(hipEventElapsedTime(&a, ev[3 * i], ev[3 * i + 1]));
            HIP_CHECK(hipEventElapsedTime(&b, ev[3 * i + 1], ev[3 * i + 2]));
            tx += a;
            ty += b;
        }
        for (auto &e : ev) (void)hipEventDestroy(e);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (total_ms) *total_ms = ms;
    if (xhalf_ms) *xhalf_ms = tx;
    if (yhalf_ms) *yhalf_ms = ty;
    return 0;
    GUARD_END(-1)
}
