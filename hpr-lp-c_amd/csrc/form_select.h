// form_select.h -- which kernel form a matrix gets (stream, fused tiled, piece form, all-remainder, long rows aside): the
// numbered rules of DESIGN.md section 3 as functions of measured facts and test hooks.  Plain host code: no HIP header, no
// HIP call.  solver.cpp measures (device kernels, host scans), asks here, builds, asks again; hprlp_form_select (abi.cpp)
// runs the same stages on a recorded facts record, so that every rule can be exercised without a GPU.
#pragma once

#include "hprlp_amd.h"

namespace hprlp {

using FormFacts = ::hprlp_form_facts;  // what the rules look at (include/hprlp_amd.h)
using FormBuilt = ::hprlp_form_built;
using FormHooks = ::hprlp_form_hooks;

// Every test hook that influences the selection, read through env_get() -- per call, not cached (env.h: the parity suite
// builds many forms in one process).
FormHooks read_form_hooks();
// a facts record with every lazily measured entry marked "not measured"
FormFacts blank_form_facts();

// The tile geometry the rules speak of, as tiled.h defines it for the kernels (tiled.h includes the HIP runtime; solver.cpp
// asserts that the two agree).
constexpr int kFormTileRows = 8192, kFormTileRowsMin = 1024, kFormTileCols = 2048, kFormTileColsNarrow = 1024;
constexpr int kFormMaxRow = 1024, kFormPbRowsMax = 4096;

constexpr int kSkewRow = 256;              // rows longer than this count as long ...
constexpr double kMaxLongRowShare = 0.2;   // ... and a matrix with more than this share of its entries in them keeps the stream kernel
constexpr double kMaxBlockLoad = 4.0;      // heaviest block of sb_rows rows / mean, above which the fused tiled forms are declined
constexpr double kPiecesMinDense = 0.75;   // share of the entries in staged tiles below which the PIECE form is declined
constexpr double kStreamLineDensity = 0.25;  // at most this many 64-byte lines gathered per entry -> stream kernel
constexpr double kStreamL2LineDensity = 0.6;  // ... and only while neighbouring rows still share lines: with a line per entry the L2 holds the window but every gather
                                              // misses the L1 (1.5M x 1.5M, band 75 000, 0.93 lines per entry: stream 0.177 ms per half-step, pieces 0.128; the
                                              // multicommodity-flow LP the rule was made for: 0.35 / 0.15)
constexpr int kTiledMinCols = 7 << 16;        // fewest columns of a matrix that is tried in a tiled form (458 752: 3.5 MiB of gathered vector)
constexpr double kStreamLineDensityLong = 0.12;  // ... lines per entry up to which rows of ANY length keep the coalesced-rows preference
constexpr double kCoalescedMaxRowEntries = 32.0;   // the coalesced-rows preference for the stream kernel holds up to this many entries per row
constexpr double kStreamL2LineDensityFused = 0.5;  // ... the same against a FUSED tiled form that needs its longest rows kept aside
constexpr double kFewRowsTileShare = 1.8;    // most tile bytes per entry byte at which a matrix of few rows is still tried in the piece form
                                             // (threshold sweep, tools/form_regret.py --corpus boundaries: piece form ahead of the all-remainder form by 12-41 % at
                                             // 0.8 / 1.2 / 1.5, level at 1.3, behind by 8-17 % at 2.2 / 2.8 and 2-3 x from 3.2 on)
constexpr double kPopularFarShare = 0.8;     // share of the remainder that 2 MB of the gathered vector serve, from which ...
constexpr double kPopularFarMinRem = 0.1;    // ... a copy with at least this share of its entries in the remainder is dropped for the stream kernel (one-L2 window)
constexpr double kPiecesThinRows = 10.0;     // below this many entries per row a PIECE-form copy is dropped for the stream kernel
constexpr double kPiecesMinRowEntries = 16.0;  // ... or while rows are thin
constexpr double kStreamL2Bytes = 3.0e6;  // an XCD's share of the gathered vector that one 4 MiB L2 keeps beside the matrix stream

// Gather vector too long for the L2s (>= 4 M entries = 32 MB) and the tiled build declined for lack of dense tiles: the
// stream kernel would pay a fabric line per gathered element (HPRLP_NO_PB_FALLBACK=1 keeps it anyway; one GPU only).
// gathered vector from which the all-remainder tiled form beats the stream kernel on a pattern without locality (measured,
// tools/unstructured_ab.py, uniformly random 10 per row: 1M columns 0.154 vs 0.125 ms per half-step, 2M 0.218 vs 0.318, 3M 0.316
// vs 0.508, 4.2M 0.46 vs 0.75, 6M 0.59 vs 1.13)
constexpr double kMaxTileShare = 0.6;  // tile_shapes: most tile bytes per entry byte a lowered super-block may stage (one round)
constexpr double kMaxTileShareRounds = 0.9;  // ... when the height only trims a partial last round of a larger matrix
constexpr long kPbMinCols = 800000;  // (round 4, tools/unstructured_ab.py with k_pb_fused, 10 per row: 0.5M columns 0.065 vs 0.041 ms stream, 1.0M 0.080 vs 0.123, 1.5M 0.119 vs 0.214: from where the vector outgrows a 4 MiB L2)
constexpr int kPbFewRowsMin = 32768;   // all_remainder_wanted: fewest rows of a matrix that takes the all-remainder form without having been through the tiled build
constexpr long kPopularLines = 32768;      // all_remainder_wanted: 2 MB of the gathered vector ...
constexpr double kPopularShareMax = 0.3;   // ... that may not take more than this share of a few-row matrix' gathers
constexpr double kPbHeaviestBlockShare = 48.0;  // all_remainder_wanted: a matrix with long rows takes the all-remainder form only if its heaviest 4096-row block holds at most 1 / 48 of the entries
constexpr int kPbFewRowsLow = 80000;    // ... half that height below this many rows
constexpr int kPbFewRowsHeight = 512;  // pb_height: super-block height for such a matrix (below 32 full-height super-blocks' worth of rows)
constexpr double kNarrowTilesFrom = 1.2;  // tile_shapes: entries of a row per 2048-column tile from which the copy gets 1024-column tiles

// Why a matrix has no tiled copy: what hprlp_solver_describe says in brackets, in the order of precedence the note has always
// had (a skewed matrix whose rows also share their lines reads "skew").  Skew .. Shape: the build was not attempted.
enum class NoTiled { None, Skew, Imbalance, Coalesced, OneL2, Shape, Sparse, Thin, Popular, FewRows };
const char *no_tiled_note(NoTiled why);  // "" or " [...]"
inline bool not_attempted_for_shape(NoTiled w) { return w >= NoTiled::Skew && w <= NoTiled::Shape; }
struct FormOutcome {
    NoTiled why = NoTiled::None;
    // not attempted for the length of its rows alone (longest row, or too many entries in long rows) -- not because its rows
    // share lines or gather from one L2's window.  Not a reason the note prints: an input of rule 13.
    bool long_rows_alone = false;
};

// A measurement that the next rule needs and the facts record does not hold yet.  The caller measures it, fills it in and asks
// again: a device pass runs only when the earlier rules have not decided.
enum class FormNeed { Nothing, HeaviestBlock, TilingShare, PopularShare, HeaviestPbBlock };

enum class FormRoute { Nothing, ThinEarly, NotAttempted, FewRows, DeviceBuild, HostBuild };

// Before the build.
struct PreBuild {
    FormNeed need = FormNeed::Nothing;  // != Nothing: the other fields are not final
    int min_rows = 0, min_cols = 0;
    double min_dense = 0.5, entries_per_row = 0.0;
    bool host_tiling = false;
    bool shape = false, coalesced = false, one_l2 = false, skew = false, imbalance = false;  // shape: the super-flag of the other four
    bool thin_early = false;  // rule 12: thin rows, and the cheap tiling test says the copy would pass -> stream kernel, no build
    bool side_open = false;   // the long-rows-aside attempt is open: count the long rows (host scan) and ask long_rows_aside()
    NoTiled shape_reason() const;
};
PreBuild before_build(const FormFacts &f, const FormHooks &h);
// few enough long rows (facts: n_long_rows, long_rows_nnz) for a copy without them
bool long_rows_aside(const FormFacts &f);
// where the set-up goes when no copy with the long rows aside was kept, and what is known by then
FormRoute route_of(const FormFacts &f, const PreBuild &p, FormOutcome *out);
// After a build (side: the copy without its long rows): None = keep it, else drop it for that reason.  far_built: the
// remainder lists are in their final form (rem_top_share is known) -- asks the popular-columns rule as well.
NoTiled after_build(const FormFacts &f, const FormHooks &h, const PreBuild &p, const FormBuilt &b, bool side, bool far_built);
double staged_share(const FormBuilt &b);  // share of the copy's entries in staged tiles

// The all-remainder decision (rules 7, 13) for a matrix whose pass left `o` and no copy (has_copy false).
struct AllRemainder {
    FormNeed need = FormNeed::Nothing;
    bool wanted = false;
    bool few_rows = false, long_rows = false;  // which rule asked (the [timing] lines)
};
AllRemainder all_remainder_wanted(const FormFacts &f, const FormHooks &h, const FormOutcome &o, bool has_copy);

// Heights and tile widths (Solver::choose_sb_rows / choose_pb_rows hold the arrays and the device; the arithmetic is here).
int whole_rounds_height(int rows, int slots);
int pb_height(int nrows, int slots);  // super-block height of the all-remainder form
bool pb_kernel_fits(int sb_rows, const FormHooks &h);
// nothing to estimate from the rows' column spans: heights forced, a row shard, or a small matrix
bool row_spans_wanted(long nnz, bool sharded, const FormHooks &h);
struct TileShapes {
    int sb_rows_a = kFormTileRows, sb_rows_at = kFormTileRows;  // far_group of A = sb_rows of A^T and vice versa
    int tile_cols_a = kFormTileCols, tile_cols_at = kFormTileCols;
    double xcd_bytes_a = 0.0, xcd_bytes_at = 0.0;
    // for the [timing] lines: estimated at all / heights weighed at all, and the figures
    bool estimated = false, weighed = false, lowered = false;
    double per_tile_a = 0.0, per_tile_at = 0.0, ratio_a = 0.0, ratio_at = 0.0;
    int ra = 0, rat = 0;
};
// median_span: median column span of a row without its outermost entries (<= 0: not sampled, or too few rows to tell)
TileShapes tile_shapes(int m, int n, long nnz, int slots, double median_span, const FormHooks &h);

// All stages on a recorded facts record (hprlp_form_select).  False + *missing when a rule asks for a fact that is not there.
bool form_select(const FormFacts &f, const FormHooks &h, ::hprlp_form_decision *out, const char **missing);

}  // namespace hprlp
