// abi_common.h -- what the files of the extern "C" boundary (abi_*.cpp) share: the handle structs, the one guard every entry
// runs under, the handle checks, the single-GPU refusal, the trace scope and the helpers more than one of those files calls.
// Private: not installed, and nothing outside abi_*.cpp includes it.
#pragma once

#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "hprlp_amd.h"
#include "batched.h"
#include "dist.h"
#include "solver.h"

struct hprlp_solver {
    hprlp::Solver s;
    hprlp::Comm *comm = nullptr;   // owned; destroyed after the solver's device state
    hprlp::Comm *xcomm = nullptr;  // owned; the exchange stream's own communicator (second unique id), may be null
    bool sharded = false;          // created by hprlp_solver_create_dist* / _local* (no infeasibility detection)
};

struct hprlp_batched_solver {
    hprlp::BatchedSolver *s = nullptr;
};

struct hprlp_local_group {
    hprlp::LocalGroup *g = nullptr;
};

namespace hprlp {

// Every entry's body runs here: an exception becomes hprlp_last_error() and the entry's fail value.  What an entry's failure
// does beyond that (a line on stderr, freeing results or certificates) is the body's own business.
template <class R, class F>
R guarded(R fail, F &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        set_last_error(e.what());
    } catch (...) {
        set_last_error("unknown exception");
    }
    return fail;
}

// The solver behind a handle; a null handle is refused with "<who>: null solver".  With `also`: an output the entry refuses in
// the same breath, "<who>: null solver / <also_name>" for either.
inline Solver &solver_of(hprlp_solver *h, const char *who) {
    if (!h) throw std::runtime_error(std::string(who) + ": null solver");
    return h->s;
}
inline Solver &solver_of(hprlp_solver *h, const char *who, const void *also, const char *also_name) {
    if (!h || !also) throw std::runtime_error(std::string(who) + ": null solver / " + also_name);
    return h->s;
}
inline BatchedSolver *solver_of(hprlp_batched_solver *h, const char *who) {
    if (!h || !h->s) throw std::runtime_error(std::string(who) + ": null solver");
    return h->s;
}
inline BatchedSolver *solver_of(hprlp_batched_solver *h, const char *who, const void *also, const char *also_name) {
    if (!h || !h->s || !also) throw std::runtime_error(std::string(who) + ": null solver / " + also_name);
    return h->s;
}

// A sharded solver is refused: "<who>: <what>; a sharded solver (hprlp_solver_create_dist* / _local*) refuses <refuses>", or
// "<who>: <what>" alone with refuses null.  Each entry's sentence is its own; h has passed solver_of.
inline void single_gpu_only(const hprlp_solver *h, const char *who, const char *what, const char *refuses = "it") {
    if (!h->sharded) return;
    std::string msg = std::string(who) + ": " + what;
    if (refuses) msg += std::string("; a sharded solver (hprlp_solver_create_dist* / _local*) refuses ") + refuses;
    throw std::runtime_error(msg);
}

// The caller's trace buffer is the solver's for the scope, however the scope is left.
struct TraceScope {
    Solver &s;
    TraceScope(Solver &solver, hprlp_trace_row *trace, int max_trace) : s(solver) {
        static_assert(sizeof(hprlp_trace_row) == sizeof(TraceRow), "trace row layout");
        s.trace = reinterpret_cast<TraceRow *>(trace);
        s.trace_cap = trace ? max_trace : 0;
    }
    ~TraceScope() {
        s.trace = nullptr;
        s.trace_cap = 0;
    }
    TraceScope(const TraceScope &) = delete;
    TraceScope &operator=(const TraceScope &) = delete;
};

// The blocks of counts, seconds and phases an entry keeps for its hprlp_last_* accessor.
inline void keep_counts(long (&block)[8], const long (&v)[8]) {
    for (int i = 0; i < 8; ++i) block[i] = v[i];
}
template <class T, int N>
int read_counts(const T (&block)[N], T *out) {
    if (!out) return -1;
    for (int i = 0; i < N; ++i) out[i] = block[i];
    return 0;
}

// abi_solve.cpp
HPRLP_results make_error_result(const char *status);
void check_start(const double *v, long len, const char *what);  // a warm start's entries must be finite (null: zeros)
bool detection_from(const hprlp_detection *d, Detection *out);  // false: d is null (off); throws for a negative eps
void clear_certificate(hprlp_certificate *c, int m, int n);
bool export_certificate(const Certificate &k, hprlp_certificate *c, int m, int n);  // false: the host allocation failed

// abi_batched.cpp
bool clear_batched_certificates(hprlp_batched_certificates *c, int B, int m, int n);           // false: the host allocation failed
bool export_batched_certificates(const std::vector<Certificate> &k, hprlp_batched_certificates *c);  // likewise

// abi_solver.cpp: the solver first (its device state, and a background tiling job, go before the transport); null is a no-op
void destroy_handle(hprlp_solver *h);

}  // namespace hprlp
