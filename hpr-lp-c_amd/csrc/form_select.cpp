// form_select.cpp -- the kernel-form selection rules (form_select.h; DESIGN.md section 3 numbers them).  Host only.
#include "form_select.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "env.h"

namespace hprlp {

FormHooks read_form_hooks() {
    FormHooks h = FormHooks();
    auto value = [](const char *e, bool real) {
        ::hprlp_form_hook_value v = {e != nullptr, 0.0};
        if (e) v.value = real ? std::atof(e) : static_cast<double>(std::atol(e));
        return v;
    };
    h.no_tiled = env_on("HPRLP_NO_TILED");
    h.tiled_anyway = env_get("HPRLP_TILED_ANYWAY") != nullptr;
    h.pieces_anyway = env_get("HPRLP_PIECES_ANYWAY") != nullptr;
    h.host_tiling = env_on("HPRLP_HOST_TILING");
    h.no_long_side = env_on("HPRLP_NO_LONG_SIDE");
    h.no_pb_fallback = env_on("HPRLP_NO_PB_FALLBACK");
    h.no_pb_long_rows = env_get("HPRLP_NO_PB_LONG_ROWS") != nullptr;
    h.no_pb_kernel = env_get("HPRLP_NO_PB_KERNEL") != nullptr;
    h.tiling_check = env_get("HPRLP_TILING_CHECK") == nullptr ? 0 : env_on("HPRLP_TILING_CHECK") ? 1 : 2;
    h.tiled_min_rows = value(env_get("HPRLP_TILED_MIN_ROWS"), false);
    h.tiled_min_dense = value(env_get("HPRLP_TILED_MIN_DENSE"), true);
    h.tiled_min_cols = value(env_get("HPRLP_TILED_MIN_COLS"), false);
    h.pb_min_cols = value(env_get("HPRLP_PB_MIN_COLS"), false);
    h.pb_min_nnz = value(env_get("HPRLP_PB_MIN_NNZ"), false);
    h.tile_rows = value(env_get("HPRLP_TILE_ROWS"), false);
    h.tile_cols = value(env_get("HPRLP_TILE_COLS"), false);
    return h;
}

FormFacts blank_form_facts() {
    FormFacts f = FormFacts();
    f.line_density = 1.0;
    f.min_dense_override = -1.0;
    f.heaviest_block = f.n_long_rows = f.long_rows_nnz = f.heaviest_pb_block = -1;
    f.tiling_share = f.popular_share = -1.0;
    f.side.ok = f.whole.ok = -1;
    return f;
}

// "No rule applies when a test forces a form", as each rule spells it.  The guards differ in which hooks they let through; the
// differences are kept as they were found.
// Rules 1, 2, 6 (skew, imbalance, coalesced rows): lets HPRLP_PIECES_ANYWAY and HPRLP_TILED_MIN_DENSE through.
static bool fused_rules_apply(const FormFacts &f, const FormHooks &h) { return !h.tiled_min_rows.set && f.min_dense_override < 0.0 && !h.tiled_anyway; }
// Rule 4 (one L2): the same and HPRLP_PIECES_ANYWAY; lets HPRLP_TILED_MIN_DENSE through.
static bool one_l2_rule_applies(const FormFacts &f, const FormHooks &h) { return fused_rules_apply(f, h) && !h.pieces_anyway; }
// Rule 11 (few rows, dense tiles): only HPRLP_TILED_MIN_ROWS and the all-remainder request turn it off.
static bool few_rows_rule_applies(const FormFacts &f, const FormHooks &h) { return !h.tiled_min_rows.set && f.min_dense_override < 0.0; }
// Rules 3, 8 on a built copy of the whole matrix: lets HPRLP_TILED_ANYWAY through.
static bool piece_rules_apply(const FormFacts &f, const FormHooks &h) {
    return !h.tiled_min_rows.set && !h.tiled_min_dense.set && f.min_dense_override < 0.0 && !h.pieces_anyway;
}
// Rules 3, 12 on a copy with its long rows aside: lets HPRLP_TILED_ANYWAY through, and the all-remainder request as well.
static bool side_piece_rules_apply(const FormHooks &h) { return !h.tiled_min_rows.set && !h.tiled_min_dense.set && !h.pieces_anyway; }
// Rule 10 (popular far entries): every forcing hook turns it off.
static bool popular_rule_applies(const FormFacts &f, const FormHooks &h) { return piece_rules_apply(f, h) && !h.tiled_anyway; }
// Rule 12 before the build (the cheap tiling test): every forcing hook, the host builder and any HPRLP_TILING_CHECK turn it off.
static bool thin_early_rule_applies(const FormFacts &f, const FormHooks &h) {
    return popular_rule_applies(f, h) && !h.host_tiling && h.tiling_check == 0;
}

static long super_blocks(const FormFacts &f) { return (f.rows + f.sb_rows - 1) / f.sb_rows; }
static bool in_one_l2(const FormFacts &f) { return f.xcd_gather_bytes > 0.0 && f.xcd_gather_bytes <= kStreamL2Bytes; }

NoTiled PreBuild::shape_reason() const {
    return skew ? NoTiled::Skew : imbalance ? NoTiled::Imbalance : coalesced ? NoTiled::Coalesced : one_l2 ? NoTiled::OneL2 : shape ? NoTiled::Shape : NoTiled::None;
}

const char *no_tiled_note(NoTiled why) {
    switch (why) {
        case NoTiled::Skew: return " [tiled form not attempted: too many entries in long rows]";
        case NoTiled::Imbalance: return " [tiled form not attempted: unbalanced row blocks]";
        case NoTiled::Coalesced: return " [tiled form not attempted: neighbouring rows gather from the same lines]";
        case NoTiled::OneL2: return " [tiled form not attempted: the stream kernel's gathers stay in one L2]";
        case NoTiled::Shape: return " [tiled form not attempted: shape]";
        case NoTiled::Sparse: return " [tiled form declined: too few entries in dense tiles]";
        case NoTiled::Thin: return " [tiled piece form declined: thin rows]";
        case NoTiled::Popular: return " [tiled form declined: its remainder gathers from a few popular columns]";
        case NoTiled::FewRows: return " [tiled form not attempted: too few rows]";
        case NoTiled::None: break;
    }
    return "";
}

double staged_share(const FormBuilt &b) {
    return static_cast<double>(b.dense_entries) / std::max(1.0, static_cast<double>(b.dense_entries) + static_cast<double>(b.n_rem));
}

// The order of the rules is part of the behaviour: each reads what the earlier ones decided.
PreBuild before_build(const FormFacts &f, const FormHooks &h) {
    PreBuild p;
    const bool mr = h.tiled_min_rows.set;
    const long rows = f.rows, cols = f.cols, nnz = f.nnz, rb = f.sb_rows;
    // column-tiled copy: only for matrices with at least one 8192-row super-block per CU and with enough column locality
    // measured on shard-shaped matrices of the banded benchmark: 305 super-blocks 0.31 ms tiled vs
    // 0.38 ms stream, 153 super-blocks 0.21 ms both -> one super-block per CU is the break-even
    // (round 2: matrices with fewer super-blocks than CUs run the split form -- several workgroups per super-block)
    // (lowered height: chosen by tile_shapes so that there is a super-block per workgroup slot)
    // (a copy asked for WITHOUT a dense-tile requirement -- the all-remainder form, all_remainder_wanted -- stages no tile:
    // the row count that makes staging pay does not apply to it)
    p.min_rows = mr ? static_cast<int>(h.tiled_min_rows.value) : f.min_dense_override >= 0.0 ? 1 : static_cast<int>(rb < kFormTileRows ? 256 * rb : 32 * kFormTileRows);
    p.min_dense = f.min_dense_override >= 0.0 ? f.min_dense_override : (h.tiled_min_dense.set ? h.tiled_min_dense.value : 0.5);
    p.host_tiling = h.host_tiling;
    // Two more conditions on the shape (measured late in round 2, tools/longrow_ab.py):
    //  * the gathered vector must be big enough for staging it to pay: a 300k x 100k matrix passes the dense-tile test but
    //    its 0.8 MB vector lives in every L2 anyway -- stream kernel 11.5 us, tiled 30.7 us per launch.  Tiled from 2^20
    //    columns on (8 MB: beyond an XCD's 4 MiB L2).  An explicit HPRLP_TILED_MIN_ROWS (tests) lifts the default.
    //  * no long rows: a row's entries beyond four per tile go to the remainder list, where ONE lane adds a row's
    //    consecutive products (two dependent LDS reads each): five rows of 3000 entries took that launch from 31 to 203
    //    us.  Such matrices keep the stream kernel, which spreads a long row over a wave or several.
    // Rule 5.  (2^19 columns = 4 MiB = one L2.  Until round 5 the full-height form waited for 800 k columns: a 600k x 600k band of 40 000
    // columns, 40 per row, kept the stream kernel at 0.25 of 8 TB/s where the piece form runs 0.33 and the lowered fused form 0.36)
    // (7 * 2^16 since the threshold sweep of round 5: 2 % band, 20 per row: 400 k columns stream 0.070 / lowered tiled 0.078 ms,
    // 500 k columns 0.098 / 0.082 -- the vector shares its L2 with the matrix stream)
    p.min_cols = h.tiled_min_cols.set ? static_cast<int>(h.tiled_min_cols.value) : (mr ? 0 : kTiledMinCols);
    // (an all-remainder copy -- min_dense_override >= 0 -- takes rows of any length: its steps add a row's products by a segmented
    // reduction over the lanes, all_remainder_wanted)
    p.shape = cols < p.min_cols || (f.longest_row > kFormMaxRow && f.min_dense_override < 0.0);
    // bytes of the vector tiles a FULL-height super-block stages against the bytes of its entries (the row span back out of
    // tile_shapes' estimate): above 1 the piece form moves more tile bytes than matrix bytes (staircase LP of 12 stages,
    // 8 entries per row, span 2.4e5 columns: pieces 0.086 ms per half-step, stream kernel 0.068)
    const double span_est = f.xcd_gather_bytes > 0.0 ? std::max(0.0, f.xcd_gather_bytes / 8.0 - cols / 8.0) : 0.0;
    const double tile_share_full =
        rows > 0 && nnz > 0 ? (span_est + static_cast<double>(kFormTileRows) * cols / rows) * 8.0 / (static_cast<double>(nnz) / rows * kFormTileRows * 11.0) : 0.0;
    // Rule 11.  Second held-out set, round 5: FEW rows (under a super-block per CU) whose full-height tiles would still be dense -- the vector
    // bytes a super-block stages stay under kFewRowsTileShare times its entries' bytes -- go through the tiled build after all and run the
    // piece form: 50k x 2M with 400 random entries per row (the transpose of a 10-per-row matrix): 7 super-blocks in 512 pieces
    // 0.101 ms per half-step, all-remainder form 0.162, stream kernel 0.291.  (100k x 5M with 150 per row: share 3.2 -- all-remainder
    // form, all_remainder_wanted.)
    if (few_rows_rule_applies(f, h) && rb == kFormTileRows && rows < p.min_rows && rows >= 4 * kFormTileRows && nnz >= 4000000 && f.xcd_gather_bytes > 0.0 &&
        tile_share_full <= kFewRowsTileShare)
        p.min_rows = static_cast<int>(rows);
    // ... and thin rows: a piece's cost goes with the tiles it stages, the stream kernel's with the entries (1M x 1M band of 16 000
    // columns, 6 per row: pieces 0.060 ms per half-step, stream 0.041; 12 per row + dense borders: 0.102 / 0.088; 20 per row: 0.128 / 0.177)
    const double entries_per_row = p.entries_per_row = rows > 0 ? static_cast<double>(nnz) / rows : 0.0;
    // Rule 6.  Rows whose neighbours gather from the same 64-byte lines (stencil rows, incidence matrices, bands a few hundred columns
    // wide) are what the stream kernel is good at: its gathers coalesce and hit the L1 / L2, and there is nothing for staged
    // tiles to save.  Measured (tools/ab_forms.sh, 1M x 1M, 20 per row): band 500 (0.1 lines per entry) stream 0.071 ms per
    // half-step, band 2000 (0.2) 0.107 -- the tiled build declines such bands (more than four entries of a row per tile) and the
    // all-remainder form that used to follow took 0.138 / 0.149; grid PDE-control LP (0.11 / 0.20): stream 0.0245 against
    // 0.0361 ms in the lowered fused form.  From 0.37 lines per entry on (band 4000) the fused tiled form wins (0.089 / 0.124).
    // (these two hold for a matrix whose longest rows would be kept aside as well: evaluated whatever the longest row is -- with the
    // layered tile lists of round 5 the copy of a block-angular LP WITHOUT its 400 linking rows passes the dense-tile test, and ran
    // 0.48 / 0.42 of 8 TB/s where the stream kernel, whose rows share their lines, runs 0.58 / 0.47)
    const bool long_only = p.shape && cols >= p.min_cols;  // declined so far for its longest row alone
    // (rows of more than kCoalescedMaxRowEntries entries excepted: the stream kernel packs 512 entries per wave, so 60-entry rows leave
    // it 8 busy lanes in its row-sum phase -- 600k x 600k, 60 per row in 6 000 columns, 0.2 lines per entry: stream 0.24 / 0.35 of
    // 8 TB/s, lowered tiled form with three layers per tile 0.42 / 0.50)
    // (... unless the rows share their lines almost completely: 1M x 1M, 40 / 48 per row inside 1 500 columns, 0.08 lines per entry:
    // stream 0.243 / 0.298 ms per iteration, lowered tiled form 0.274 / 0.359 -- threshold sweep, round 5)
    if ((!p.shape || long_only) && f.line_density <= kStreamLineDensity && (entries_per_row <= kCoalescedMaxRowEntries || f.line_density <= kStreamLineDensityLong) &&
        fused_rules_apply(f, h))
        p.shape = p.coalesced = true;
    {
        // Rule 4.  Round 4, late.  A matrix of fewer full-height super-blocks than workgroup slots whose height could not be lowered (its
        // rows' column windows are too wide for short super-blocks) would run the piece form: partial sums through memory and a
        // finish launch.  When the stream kernel's gathers stay inside one L2 anyway -- every XCD runs a contiguous eighth of the
        // rows, whose columns (median row span + the eighth's own drift along the diagonal, tile_shapes) cover less
        // than kStreamL2Bytes of the vector -- the stream kernel is the faster form: multicommodity-flow LP, 535 k x 2.03 M,
        // 40 diagonal blocks: y-half 64.9 us (512 pieces of 66 super-blocks) against 22.4 us, 10.1 k -> 18.0 k iterations/s.
        // Config 5's quarter shard (window 4.0 MB: pieces 0.31 ms, stream 0.38) keeps the pieces.
        // (a matrix of exactly `slots` super-blocks counts as fused here, as pieces in rules 2 and 12 below)
        const bool pieces_expected = rb == kFormTileRows && super_blocks(f) < f.slots;
        // pieces: round 4's rule with round 5's conditions.  A FUSED tiled form only where the copy would need its longest rows kept
        // aside (two more launches per half-step for them) and the stream kernel's rows share their lines inside one L2:
        // block-angular LP without its 400 linking rows (0.39 lines per entry, 2 MB per XCD): fused 1984-row form + side 0.48 / 0.42
        // of 8 TB/s, stream kernel 0.58 / 0.47.  (A band of 4 000 columns has the same line density and window and no long rows:
        // fused form 0.51, stream kernel 0.36.)
        const bool stream_wins = pieces_expected ? (f.line_density <= kStreamL2LineDensity || tile_share_full > 1.0 || entries_per_row < kPiecesMinRowEntries)
                                                 : (long_only && f.line_density <= kStreamL2LineDensityFused);
        if ((!p.shape || (long_only && !p.coalesced)) && in_one_l2(f) && stream_wins && one_l2_rule_applies(f, h)) p.shape = p.one_l2 = true;
    }
    // Rules 1, 2.  Round 5, from the form-regret corpus (tools/form_regret.py, profiles/r05_form_regret.txt) -- two properties of the ROW
    // LENGTHS that the tiled forms do not survive, whatever the columns look like:
    //  * skew: a matrix with a fifth of its entries in rows of more than kSkewRow entries (R-MAT / Kronecker graphs: 40 %).  A
    //    long row's entries beyond four per tile all go through the remainder steps of ONE super-block; the stream kernel
    //    gives such a row a wave of its own.  Kronecker 2^20 x 2^20, 7.5e6 entries, y-half: piece form 0.67 ms, lowered fused
    //    0.54-0.58, all-remainder 0.71, stream kernel 0.076.
    //  * imbalance: the heaviest block of sb_rows consecutive rows holds more than kMaxBlockLoad times the mean (a few hundred
    //    coupling rows at the end of a block-diagonal model).  A fused launch ends when its heaviest super-block does:
    //    block-diagonal 1M x 1.2M with 300 rows of 900 entries behind it, y-half 0.295 ms (1984-row super-blocks) against
    //    0.066 with the stream kernel.  (The piece form cuts its work evenly and is exempt.)
    const bool pieces_expected = rb == kFormTileRows && super_blocks(f) <= f.slots;
    if (fused_rules_apply(f, h)) {
        if (f.long_row_share > kMaxLongRowShare) {  // (also for a matrix whose longest rows would be kept aside, and on top of rules 4 and 6)
            p.shape = p.skew = true;
        } else if (!p.shape && rows > 100000) {
            if (!pieces_expected && f.heaviest_block < 0) return p.need = FormNeed::HeaviestBlock, p;
            const long heaviest = pieces_expected ? 0 : f.heaviest_block;
            if (static_cast<double>(heaviest) > kMaxBlockLoad * static_cast<double>(nnz) / super_blocks(f)) p.shape = p.imbalance = true;
        }
    }
    // Rule 12.  Thin rows (rule 8, after the build: a PIECE-form copy of a matrix with under kPiecesThinRows entries per row is dropped
    // for the stream kernel) decided BEFORE the build where the cheap tiling test (a sort of the entries' tile keys, under a
    // millisecond; the locality ordering's acceptance test) already says the copy would pass: the build and its drop were
    // 20-65 ms per matrix of a 0.5 s solve (two-stage LP: 0.126 s of 0.57).
    if ((!p.shape || long_only) && pieces_expected && rows >= p.min_rows && nnz > 0 && entries_per_row < kPiecesThinRows && thin_early_rule_applies(f, h)) {
        if (f.tiling_share < 0.0) return p.need = FormNeed::TilingShare, p;
        if (f.tiling_share >= kPiecesMinDense) return p.thin_early = true, p;
    }
    // A FEW long rows (dense LP columns / rows) do not have to cost the matrix the tiled kernel: they are left out of the
    // tiled copy and summed by the stream kernel's vector / split-row mode into a base vector that every tiled launch
    // adds (tiled.h: TiledDev::side_*).  At most 0.1 % of the rows (and 64) and a fifth of the nonzeros.  (Rule 6: not behind
    // the skew, coalesced-rows or one-L2 preference for the stream kernel.)
    p.side_open = cols >= p.min_cols && f.longest_row > kFormMaxRow && rows >= p.min_rows && nnz > 0 && !h.host_tiling && !h.no_long_side && !p.skew && !p.coalesced && !p.one_l2;
    return p;
}

bool long_rows_aside(const FormFacts &f) { return f.n_long_rows <= std::max<long>(64, f.rows / 1000) && f.long_rows_nnz * 5 <= f.nnz; }

FormRoute route_of(const FormFacts &f, const PreBuild &p, FormOutcome *out) {
    *out = FormOutcome();
    if (p.thin_early) {
        out->why = p.shape ? p.shape_reason() : NoTiled::Thin;
        return FormRoute::ThinEarly;
    }
    if (p.shape) {
        out->why = p.shape_reason();
        // declined for its row lengths alone (longest row, or too many entries in long rows) -- not because its rows share lines or
        // gather from one L2's window: a candidate for the all-remainder form where the COLUMNS are not popular (all_remainder_wanted)
        out->long_rows_alone = f.cols >= p.min_cols && f.longest_row > kFormMaxRow && !p.coalesced && !p.one_l2 && !p.imbalance && f.rows > 0 && f.nnz > 0;
        return FormRoute::NotAttempted;
    }
    if (f.rows < p.min_rows) {
        if (f.rows > 0 && f.nnz > 0) out->why = NoTiled::FewRows;  // (rule 7)
        return FormRoute::FewRows;
    }
    if (f.rows > 0 && f.nnz > 0) return p.host_tiling ? FormRoute::HostBuild : FormRoute::DeviceBuild;
    return FormRoute::Nothing;
}

NoTiled after_build(const FormFacts &f, const FormHooks &h, const PreBuild &p, const FormBuilt &b, bool side, bool far_built) {
    if (b.ok <= 0) return NoTiled::Sparse;  // rows >= min_rows here: what was missing is dense tiles
    // Rule 3.  Round 5 (form-regret corpus): the PIECE form of a copy that stages only about half of its entries is the worst of both
    // worlds -- every super-block's remainder steps stay with one piece, the partial sums go through memory.  Uniform random
    // 1.2M x 1.2M, 16 per row (51 % in tiles): 0.55 ms per iteration against 0.27 in the all-remainder form; band + 30 % far
    // entries (53 %): 0.39 against 0.28.  Such a copy is handed back as "too few entries in dense tiles": the
    // all-remainder form follows where the matrix is large enough for it (all_remainder_wanted), else the stream kernel.
    if (b.n_pieces > 0 && (side ? side_piece_rules_apply(h) : piece_rules_apply(f, h))) {
        if (staged_share(b) < kPiecesMinDense) return NoTiled::Sparse;
        // Rule 8 (rule 12 for the copy with its long rows aside).  Held-out corpus, round 5: a copy that passes the dense-tile test has
        // its rows' columns close together -- and
        // with fewer than ten entries per row the stream kernel then beats the PIECE form whether or not an XCD's window
        // fits its L2 (a piece's cost goes with the tiles it stages): node-arc incidence 1M x 4M after the locality
        // ordering, 8 / 2 per row: 0.070 / 0.093 ms per half-step in pieces, 0.055 / 0.085 on the stream kernel; 5-, 7-
        // and 9-point stencils in random order (after the ordering) 5-13 % per iteration; 3M x 3M band of 300 000 columns,
        // 8 per row: 0.357 -> 0.327 ms (12 per row: pieces stay ahead, 0.275 against 0.293).
        if (p.entries_per_row < kPiecesThinRows) return NoTiled::Thin;
    }
    // Rule 10 (not asked of a copy with its long rows aside).  Second held-out set, round 5: what the tiles could not hold gathers from a
    // FEW popular columns (the first-stage columns of
    // a two-stage stochastic LP: 20 % of the entries, 160 KB of the vector) and the rest of a row from a window that an XCD's L2
    // holds anyway: the stream kernel finds ALL of it in its L2, the tiled form sends the popular fifth through the remainder at
    // 30 bytes per entry.  1M x 1.42M, 8 per row, 2 000 scenario blocks: lowered fused form 0.080 ms per half-step (28 % in
    // the remainder), stream kernel 0.034.  (A band with 30 % uniformly far entries has the same share in the remainder and NO
    // such concentration: the tiled form stays ahead, 0.237 against 0.288 ms per iteration.)
    if (!side && far_built && in_one_l2(f) && popular_rule_applies(f, h) && static_cast<double>(b.n_rem) >= kPopularFarMinRem * static_cast<double>(f.nnz) &&
        b.rem_top_share >= kPopularFarShare)
        return NoTiled::Popular;
    return NoTiled::None;
}

AllRemainder all_remainder_wanted(const FormFacts &f, const FormHooks &h, const FormOutcome &o, bool has_copy) {
    AllRemainder r;
    if (h.no_pb_fallback || h.no_tiled) return r;
    const long min_cols = h.pb_min_cols.set ? static_cast<long>(h.pb_min_cols.value) : kPbMinCols;
    const long min_nnz = h.pb_min_nnz.set ? static_cast<long>(h.pb_min_nnz.value) : 4000000L;  // (tests lower it)
    // a pattern whose rows stay near a diagonal keeps the stream kernel: each XCD's eighth of the rows gathers from a window of the
    // vector that its L2 holds (tile_shapes: xcd_gather_bytes; 0 = not estimated).  1M x 1M, band 2000, 20 per row (the
    // tiled build declines it: too many entries of a row per tile): stream 0.107 ms per half-step, all-remainder form 0.149.
    const bool in_l2 = in_one_l2(f) && !h.pb_min_cols.set;
    // Rule 7.  Round 5, held-out corpus (tools/form_regret.py --corpus held_out): a matrix with FEWER rows than the staged forms ask for
    // (a super-block per CU) never reached the tiled build, so it never got here either -- and kept the stream kernel at 0.11 of
    // 8 TB/s where its rows gather at random from millions of columns: 200k x 5M with 75 per row (the transpose of a 3-per-row
    // matrix), x-half 0.262 ms against 0.125 here (pre-pass 0.073 + k_pb_fused 0.049, super-blocks of 512 rows); 100k x 5M with
    // 150 per row: 0.262 against 0.140.  Taken where the rows do NOT share their lines (line_density).
    // ... and where a ROW's own column window is beyond an L2 (xcd_gather_bytes less the drift of the eighth along the diagonal =
    // the median row span): 150k x 3M with 60 per row inside a window of 150 000 columns has every entry on a line of its own and
    // still gathers out of 1.2 MB -- stream kernel 0.063 ms, all-remainder form 0.081.
    const double row_window_bytes = f.xcd_gather_bytes > 0.0 ? f.xcd_gather_bytes - static_cast<double>(f.cols) : 0.0;
    r.few_rows = o.why == NoTiled::FewRows && f.rows >= kPbFewRowsMin && f.line_density >= kStreamL2LineDensity &&
                 (f.xcd_gather_bytes <= 0.0 || row_window_bytes > kStreamL2Bytes);
    const bool size_ok = !f.sharded && !has_copy && !in_l2 && f.cols >= min_cols && f.nnz >= min_nnz;
    const bool sparse = o.why == NoTiled::Sparse;
    // Rule 13.  Validation set, end of round 5: a matrix kept off the tiled forms for its LONG rows (hubs of a b-matching LP: rows of up to 77 000
    // entries, a quarter of the entries in rows over 1 024) whose columns are NOT popular gathers at random like any unstructured
    // matrix -- stream kernel 0.12 of 8 TB/s.  k_pb_fused adds rows of any length; what it cannot take is a super-block far heavier
    // than the chip's share (the launch ends with it).  (A Kronecker graph has popular columns: it keeps the stream kernel, rule 1.)
    if (o.long_rows_alone && size_ok && !sparse && !r.few_rows && f.line_density >= kStreamL2LineDensity && !h.no_pb_long_rows) {
        if (f.popular_share < 0.0) return r.need = FormNeed::PopularShare, r;
        if (f.heaviest_pb_block < 0) return r.need = FormNeed::HeaviestPbBlock, r;
        r.long_rows = f.popular_share <= kPopularShareMax && static_cast<double>(f.heaviest_pb_block) * kPbHeaviestBlockShare <= static_cast<double>(f.nnz);
    }
    if (r.long_rows) return r.wanted = true, r;
    if (r.few_rows && size_ok && !sparse) {
        // ... and where no small set of popular columns takes a large share of the gathers (they stay in the L2s whatever the rows'
        // reach): set-covering pattern 200k x 2M, 50 per row, column popularity ~ c^-0.6 -- 44 % of the entries on the 32 768 most
        // popular lines (2 MB): stream kernel 0.123 ms, all-remainder form 0.144 (uniform columns: 5 %).
        if (f.popular_share < 0.0) return r.need = FormNeed::PopularShare, r;
        if (f.popular_share > kPopularShareMax) r.few_rows = false;
    }
    r.wanted = size_ok && (sparse || r.few_rows);
    return r;
}

// Super-block heights of an LP's tiled copies (tiled.h).  A matrix with fewer than 512 full-height super-blocks cannot give
// every workgroup slot of the chip a whole super-block: it ran the piece form (three launches, partial sums through memory) or,
// below 2^20 columns, the stream kernel.  With R = rows / 512 every slot gets exactly one, the epilogue stays fused, a half-step
// is one launch and there is no tail.  What a lower super-block costs is tile traffic -- a staged tile serves R rows -- so the
// column window of a super-block must stay narrow against its entries: estimated from the column span of the middle three quarters of the
// entries of 2048 sampled rows (the far entries of a band matrix do not count: they go through the remainder lists).  A
// source group of one matrix' remainder lists is a super-block of the other (hand-off, kernels.h FarPush): far_group of A is
// sb_rows of A^T and vice versa.  Same-box A/B (profiles/r03_ab_rows*.txt): 1M x 1M, band 1e4: 3658 it/s stream kernel, 3393
// pieces, 5287 with 2048-row super-blocks; the 1.25M x 10M shard of config 5 (window of 2e5 columns): a loss, declined here.
// The height that fills exactly k rounds of the chip's workgroup slots, k = the rounds the FULL height needs (k = 1: one
// super-block per slot); the full height where its rounds are nearly full already.
int whole_rounds_height(int rows, int slots) {
    const int nsb_full = (rows + kFormTileRows - 1) / kFormTileRows;
    const int k = std::max(1, (nsb_full + slots - 1) / slots);
    if (k > 1 && static_cast<double>(nsb_full) / (static_cast<double>(k) * slots) >= 0.8) return kFormTileRows;  // rounds nearly full already
    const int per = (rows + k * slots - 1) / (k * slots);
    return std::min(kFormTileRows, (per + 63) / 64 * 64);
}

// Height for a matrix that runs the tiled form WITHOUT staged tiles (all_remainder_wanted: every entry through the
// propagation-blocking remainder).  No tile is staged, so a lower super-block costs nothing in tile traffic: take the height
// that gives every workgroup slot whole super-blocks -- the half-step is then ONE fused launch whose epilogue hands the
// products over to the other half (round 3 ran such matrices at full height: 245 super-blocks of a 2M x 2M matrix = the piece
// form, three launches per half-step, partial sums through memory, no hand-off).  HPRLP_TILE_ROWS still overrides.
// At most kFormPbRowsMax rows (the all-remainder kernel's accumulators, kernels.hip: k_pb_fused): larger matrices take more rounds.
int pb_height(int nrows, int slots) {
    // (few rows: 512-row super-blocks measured best -- 200k rows: 256 / 384 / 512 / 1024 rows 0.166 / 0.148 / 0.125 / 0.142 ms,
    // 100k rows: 0.160 / 0.153 / 0.140 / 0.193)
    // (50k rows: 256 / 512 rows 0.170 / 0.182; 33k rows: 0.155 / 0.190)
    if (nrows < 32 * kFormTileRows) return nrows < kPbFewRowsLow ? kPbFewRowsHeight / 2 : kPbFewRowsHeight;
    int r = std::max(kFormTileRowsMin, whole_rounds_height(nrows, slots));
    for (int k = 2; r > kFormPbRowsMax; ++k) r = std::max(kFormTileRowsMin, ((nrows + k * slots - 1) / (k * slots) + 63) / 64 * 64);
    return r;
}

// (HPRLP_NO_PB_KERNEL, A/B runs: the all-remainder copy through k_tiled_fused's remainder steps, as in round 3)
bool pb_kernel_fits(int sb_rows, const FormHooks &h) { return sb_rows <= kFormPbRowsMax && !h.no_pb_kernel; }

// (a row shard holds all columns of the LP against 1 / P of the rows: full height)
bool row_spans_wanted(long nnz, bool sharded, const FormHooks &h) { return !h.tile_rows.set && !sharded && nnz >= 4000000; }

TileShapes tile_shapes(int m, int n, long nnz, int slots, double median_span, const FormHooks &h) {
    TileShapes t;
    if (h.tile_cols.set)  // tests / A/B runs: one tile width for both matrices
        t.tile_cols_a = t.tile_cols_at = static_cast<int>(h.tile_cols.value) <= kFormTileColsNarrow ? kFormTileColsNarrow : kFormTileCols;
    if (h.tile_rows.set) {  // tests / A/B runs: one height for both matrices
        t.sb_rows_a = t.sb_rows_at = std::max(64, std::min(kFormTileRows, static_cast<int>(h.tile_rows.value) / 64 * 64));
        return t;
    }
    if (median_span <= 0.0) return t;
    t.estimated = true;
    const double w_a = median_span;
    const double slope = static_cast<double>(n) / m;  // columns per row along the "diagonal"
    // what one XCD's eighth of the rows gathers from (stream kernel; before_build weighs it against the piece form)
    t.xcd_bytes_a = (w_a + m / 8.0 * slope) * 8.0;
    t.xcd_bytes_at = (w_a / slope + n / 8.0 / slope) * 8.0;
    // Tile width (round 4).  A row segment of more than kTileChunk entries in one tile goes to the remainder lists WHOLE (34
    // bytes of traffic per entry against 11 in a tile).  With d entries per row spread over a window of w columns a tile of T
    // columns holds d T / w of them on average; from about 1.2 on, segments of five and more are common (1M x 1M, band 1e4,
    // d = 19: 1.95 per 2048-column tile, 10.5 % of the entries in such segments; 1024 columns: 1.2 %).  Narrow tiles halve
    // the staged bytes per step and leave the number of steps about the same (the wide tiles of such a matrix take two).
    t.per_tile_a = static_cast<double>(nnz) / m * kFormTileCols / w_a;
    t.per_tile_at = static_cast<double>(nnz) / n * kFormTileCols / std::max(w_a / slope, 1.0);
    if (!h.tile_cols.set) {
        if (t.per_tile_a > kNarrowTilesFrom) t.tile_cols_a = kFormTileColsNarrow;
        if (t.per_tile_at > kNarrowTilesFrom) t.tile_cols_at = kFormTileColsNarrow;
    }
    // Heights considered for a matrix of `rows` rows: with k = the rounds the FULL height needs (ceil of its super-blocks over the
    // slots), the height that fills exactly k rounds.  k = 1: one super-block per slot (mid-size matrices).  k >= 2: the same
    // number of rounds as now without the partial last one -- only when the full height wastes more than a fifth of its rounds
    // (6M x 6M, band 6e4: 733 super-blocks = 1.43 rounds run as 2; 1020 of 5888 rows: 1121 -> 1148 it/s; 5M x 5M: 1264 -> 1321;
    // profiles/r03_ab_rows7.txt).  Nothing to gain below kFormTileRowsMin (launch-bound matrices: the stream kernel).
    const int ra = t.ra = whole_rounds_height(m, slots), rat = t.rat = whole_rounds_height(n, slots);
    if ((ra >= kFormTileRows && rat >= kFormTileRows) || ra < kFormTileRowsMin || rat < kFormTileRowsMin) return t;
    t.weighed = true;
    // bytes of the vector tiles a super-block stages against the bytes of its entries; a height that only trims a partial round
    // may stage a little more (it saves a fifth of the rounds or more)
    t.ratio_a = (w_a + ra * slope) * 8.0 / (static_cast<double>(nnz) / m * ra * 11.0);
    t.ratio_at = (w_a / slope + rat / slope) * 8.0 / (static_cast<double>(nnz) / n * rat * 11.0);
    const bool multi = static_cast<long>(ra) * slots < m || static_cast<long>(rat) * slots < n;  // more than one round
    const double most = multi ? kMaxTileShareRounds : kMaxTileShare;
    t.lowered = t.ratio_a <= most && t.ratio_at <= most;
    if (t.lowered) {
        t.sb_rows_a = ra;
        t.sb_rows_at = rat;
    }
    return t;
}

bool form_select(const FormFacts &f, const FormHooks &h, ::hprlp_form_decision *d, const char **missing) {
    static const char *const kNeedName[] = {"", "heaviest_block", "tiling_share", "popular_share", "heaviest_pb_block"};
    *d = ::hprlp_form_decision();
    FormOutcome o;
    if (!h.no_tiled) {  // (with HPRLP_NO_TILED=1 the set-up leaves the matrix as it is: stream kernel, no note)
        const PreBuild p = before_build(f, h);
        if (p.need != FormNeed::Nothing) return *missing = kNeedName[static_cast<int>(p.need)], false;
        d->min_rows = p.min_rows;
        d->min_cols = p.min_cols;
        d->min_dense = p.min_dense;
        const FormBuilt *kept = nullptr;
        if (p.side_open && !p.thin_early) {
            if (f.n_long_rows < 0) return *missing = "n_long_rows", false;
            if (long_rows_aside(f)) {
                if (f.side.ok < 0) return *missing = "side", false;
                d->side_tried = 1;
                if (after_build(f, h, p, f.side, true, false) == NoTiled::None) kept = &f.side;
            }
        }
        if (kept) {
            d->route = 6;
        } else {
            const FormRoute route = route_of(f, p, &o);
            d->route = static_cast<int>(route);
            if (route == FormRoute::DeviceBuild) {
                if (f.whole.ok < 0) return *missing = "whole", false;
                o.why = after_build(f, h, p, f.whole, false, true);
                if (o.why == NoTiled::None) kept = &f.whole;
            }
        }
        if (kept) {
            d->kept = 1;
            d->form = kept->n_pieces > 0 ? 2 : f.min_dense_override >= 0.0 && pb_kernel_fits(static_cast<int>(f.sb_rows), h) ? 3 : 1;
        }
    }
    d->why = static_cast<int>(o.why);
    d->long_rows_alone = o.long_rows_alone;
    std::snprintf(d->note, sizeof d->note, "%s", no_tiled_note(o.why));
    const AllRemainder ar = all_remainder_wanted(f, h, o, d->kept != 0);
    if (ar.need != FormNeed::Nothing) return *missing = kNeedName[static_cast<int>(ar.need)], false;
    d->all_remainder_wanted = ar.wanted;
    return true;
}

}  // namespace hprlp
