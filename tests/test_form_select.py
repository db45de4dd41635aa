"""The kernel-form selection rules (csrc/form_select.h) without a GPU: hprlp_form_select takes the facts a
set-up measures and returns the staged decisions.

* Replay: tests/golden/form_facts.json holds the facts of the 119 form-regret corpus patterns (A and A^T) as measured on an
  MI355X, with the form and bracketed note that the PARENT commit's library described for the same matrix.
* One constructed record on either side of each rule's threshold, thresholds as DESIGN.md section 3 states them.
* What the three "piece form expected" comparisons do for a matrix of exactly one super-block per workgroup slot.
"""
import json
import math
import os

import pytest

from conftest import hprlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "form_facts.json")

SLOTS, SB = 512, 8192  # 256 CUs x 2 resident workgroups; full super-block height
NOTE = {
    "skew": " [tiled form not attempted: too many entries in long rows]",
    "imbalance": " [tiled form not attempted: unbalanced row blocks]",
    "coalesced": " [tiled form not attempted: neighbouring rows gather from the same lines]",
    "one_l2": " [tiled form not attempted: the stream kernel's gathers stay in one L2]",
    "shape": " [tiled form not attempted: shape]",
    "sparse": " [tiled form declined: too few entries in dense tiles]",
    "thin": " [tiled piece form declined: thin rows]",
    "popular": " [tiled form declined: its remainder gathers from a few popular columns]",
    "few_rows": " [tiled form not attempted: too few rows]",
}
ROUTE = {"nothing": 0, "thin_early": 1, "not_attempted": 2, "few_rows": 3, "device_build": 4, "host_build": 5, "side_kept": 6}


def built(pieces=0, dense=0.9, nnz=100_000_000, top=0.1):
    d = int(round(dense * nnz))
    return dict(ok=1, n_pieces=pieces, dense_entries=d, n_rem=nnz - d, rem_top_share=top)


def big(**kw):
    """5M x 5M, 20 per row, 611 super-blocks (more than the slots: fused form), rows apart, window beyond an L2: builds and keeps."""
    nnz = kw.get("nnz", 100_000_000)
    f = dict(rows=5_000_000, cols=5_000_000, nnz=nnz, longest_row=40, long_row_share=0.0, line_density=0.9, xcd_gather_bytes=8.0e6,
             sb_rows=SB, slots=SLOTS, heaviest_block=nnz // 611, whole=built(nnz=nnz))
    f.update(kw)
    return f


def mid(**kw):
    """3M x 3M, 20 per row, 367 full-height super-blocks (fewer than the slots: piece form)."""
    nnz = kw.get("nnz", 60_000_000)
    f = dict(rows=3_000_000, cols=3_000_000, nnz=nnz, longest_row=40, line_density=0.9, xcd_gather_bytes=8.0e6, sb_rows=SB, slots=SLOTS,
             whole=built(pieces=512, nnz=nnz))
    f.update(kw)
    return f


def sel(f, **hooks):
    return hprlp.form_select(f, hooks)


def test_base_records_build_and_keep():
    d = sel(big())
    assert (d["route"], d["kept"], d["form"], d["note"]) == (ROUTE["device_build"], 1, "fused", "")
    assert (d["min_rows"], d["min_cols"], d["min_dense"]) == (32 * SB, 7 << 16, 0.5)
    d = sel(mid())
    assert (d["route"], d["kept"], d["form"], d["note"]) == (ROUTE["device_build"], 1, "pieces", "")


def test_rule_1_skew():
    """More than a fifth of the entries in rows of more than 256 entries -> stream kernel."""
    assert sel(big(long_row_share=0.2))["kept"] == 1
    d = sel(big(long_row_share=math.nextafter(0.2, 1.0)))
    assert (d["route"], d["kept"], d["note"]) == (ROUTE["not_attempted"], 0, NOTE["skew"])
    # on top of the coalesced-rows preference the note still reads "skew"
    assert sel(big(long_row_share=0.21, line_density=0.2))["note"] == NOTE["skew"]
    # a forced form lifts the rule
    assert sel(big(long_row_share=0.5), tiled_anyway=1)["kept"] == 1


def test_rule_2_imbalance():
    """The heaviest block of sb_rows rows holds more than 4 x the mean -> no fused tiled form; the piece form is exempt."""
    nnz, nsb = 100_000_000, 611
    edge = 4 * nnz // nsb  # floor(4 x mean)
    assert sel(big(heaviest_block=edge))["kept"] == 1
    d = sel(big(heaviest_block=edge + 1))
    assert (d["route"], d["note"]) == (ROUTE["not_attempted"], NOTE["imbalance"])
    assert sel(mid(heaviest_block=-1))["kept"] == 1  # (pieces: the block pass does not even run)
    # asked only of a matrix that the earlier rules have not declined: rows sharing their lines are "coalesced", no block pass
    assert sel(big(line_density=0.2, heaviest_block=-1))["note"] == NOTE["coalesced"]
    with pytest.raises(RuntimeError, match="heaviest_block"):
        sel(big(heaviest_block=-1))


def test_rule_3_pieces_need_tiles():
    """The piece form of a copy with under 75 % of its entries in staged tiles is handed back as too sparse."""
    assert sel(mid(whole=built(pieces=512, dense=0.75, nnz=60_000_000)))["form"] == "pieces"
    f = mid(whole=dict(ok=1, n_pieces=512, dense_entries=45_000_000 - 1, n_rem=15_000_000 + 1, rem_top_share=0.0))
    d = sel(f)
    assert (d["kept"], d["note"], d["all_remainder_wanted"]) == (0, NOTE["sparse"], 1)  # (3M columns: the all-remainder form follows)
    assert sel(dict(f, cols=799_999, xcd_gather_bytes=8.0e6))["all_remainder_wanted"] == 0  # under 800 k columns: stream kernel
    assert sel(big(whole=built(pieces=0, dense=0.6)))["form"] == "fused"  # a fused copy may stage less
    assert sel(f, pieces_anyway=1)["form"] == "pieces"


def test_rule_4_one_l2():
    """Stream kernel over pieces where an XCD's window fits one L2 (3 MB) and the rows share lines (<= 0.6 per entry), the
    full-height tiles outweigh the entries, or the rows are thin (under 16 entries)."""
    assert sel(mid(xcd_gather_bytes=3.0e6, line_density=0.6))["note"] == NOTE["one_l2"]
    assert sel(mid(xcd_gather_bytes=3.0e6 + 1, line_density=0.6))["kept"] == 1
    assert sel(mid(xcd_gather_bytes=3.0e6, line_density=math.nextafter(0.6, 1.0)))["kept"] == 1
    assert sel(mid(xcd_gather_bytes=3.0e6, nnz=16 * 3_000_000, whole=built(pieces=512, nnz=48_000_000)))["kept"] == 1
    assert sel(mid(xcd_gather_bytes=3.0e6, nnz=16 * 3_000_000 - 1))["note"] == NOTE["one_l2"]
    # the tiles of a full-height super-block outweigh its entries: share = (span + 8192 cols / rows) * 8 / (nnz / rows * 8192 * 11)
    # above 1, span = xcd_gather_bytes / 8 - cols / 8.  600k x 200k, 16 per row, rows apart:
    rows, cols, nnz = 600_000, 200_000, 9_600_000
    xcd_for = lambda share: 8.0 * (share * (nnz / rows * SB * 11.0) / 8.0 - SB * cols / rows) + cols  # noqa: E731
    f = dict(rows=rows, cols=cols, nnz=nnz, line_density=0.9, sb_rows=SB, slots=SLOTS, whole=built(pieces=512, nnz=nnz))
    assert xcd_for(1.01) < 3.0e6
    assert sel(dict(f, xcd_gather_bytes=xcd_for(1.01)), tiled_min_cols=0)["note"] == NOTE["one_l2"]
    assert sel(dict(f, xcd_gather_bytes=xcd_for(0.99)), tiled_min_cols=0)["kept"] == 1
    assert sel(mid(xcd_gather_bytes=3.0e6, line_density=0.6), pieces_anyway=1)["kept"] == 1
    # not against a fused form (611 super-blocks) without long rows
    assert sel(big(xcd_gather_bytes=3.0e6, line_density=0.4))["kept"] == 1


def test_rule_5_fewest_columns():
    """Tiled forms from 7 * 2^16 columns on."""
    assert sel(big(cols=7 << 16))["kept"] == 1
    d = sel(big(cols=(7 << 16) - 1))
    assert (d["route"], d["note"], d["long_rows_alone"]) == (ROUTE["not_attempted"], NOTE["shape"], 0)
    assert sel(big(cols=100_000), tiled_min_rows=1)["kept"] == 1  # (an explicit row threshold lifts the default)


def test_rule_6_coalesced_rows():
    """At most 0.25 lines per entry -> stream kernel; rows of more than 32 entries only up to 0.12; asked before a copy with
    its long rows aside is tried, as is the one-L2 preference (against a fused form: up to 0.5 lines per entry)."""
    assert sel(big(line_density=0.25))["note"] == NOTE["coalesced"]
    assert sel(big(line_density=math.nextafter(0.25, 1.0)))["kept"] == 1
    r = 5_000_000
    assert sel(big(line_density=0.2, nnz=32 * r, whole=built(nnz=32 * r), heaviest_block=1))["note"] == NOTE["coalesced"]
    assert sel(big(line_density=0.2, nnz=32 * r + 1, whole=built(nnz=32 * r + 1), heaviest_block=1))["kept"] == 1
    assert sel(big(line_density=0.12, nnz=33 * r))["note"] == NOTE["coalesced"]
    long_rows = dict(longest_row=2000, n_long_rows=10, long_rows_nnz=20_000, side=built())
    d = sel(big(**long_rows))
    assert (d["route"], d["side_tried"], d["kept"], d["form"]) == (ROUTE["side_kept"], 1, 1, "fused")
    d = sel(big(line_density=0.2, **long_rows))
    assert (d["side_tried"], d["note"], d["long_rows_alone"]) == (0, NOTE["coalesced"], 0)
    d = sel(big(line_density=0.5, xcd_gather_bytes=3.0e6, **long_rows))
    assert (d["side_tried"], d["note"]) == (0, NOTE["one_l2"])
    assert sel(big(line_density=math.nextafter(0.5, 1.0), xcd_gather_bytes=3.0e6, **long_rows))["route"] == ROUTE["side_kept"]
    # too many long rows for a copy without them (0.1 % of the rows, a fifth of the entries): shape, for the row lengths alone
    d = sel(big(longest_row=2000, n_long_rows=5001, long_rows_nnz=20_000_000, popular_share=0.9, heaviest_pb_block=1))  # (rule 13 asks on)
    assert (d["side_tried"], d["note"], d["long_rows_alone"]) == (0, NOTE["shape"], 1)
    assert sel(big(longest_row=2000, n_long_rows=5000, long_rows_nnz=20_000_000, side=built()))["route"] == ROUTE["side_kept"]
    assert sel(big(longest_row=2000, n_long_rows=5000, long_rows_nnz=20_000_001, popular_share=0.9, heaviest_pb_block=1))["side_tried"] == 0


def few(**kw):
    """200k x 5M, 75 per row: fewer rows than a super-block per CU, window not estimated."""
    f = dict(rows=200_000, cols=5_000_000, nnz=15_000_000, longest_row=100, line_density=0.9, xcd_gather_bytes=0.0, sb_rows=SB, slots=SLOTS,
             popular_share=0.05)
    f.update(kw)
    return f


def test_rule_7_few_rows_random_columns():
    """Fewer rows than the staged forms ask for: all-remainder form where the rows do not share lines (>= 0.6 per entry), a row's
    window is beyond an L2, at least 32 768 rows, and 32 768 popular lines take at most 30 % of the gathers."""
    d = sel(few())
    assert (d["route"], d["note"], d["all_remainder_wanted"]) == (ROUTE["few_rows"], NOTE["few_rows"], 1)
    assert sel(few(popular_share=0.3))["all_remainder_wanted"] == 1
    assert sel(few(popular_share=math.nextafter(0.3, 1.0)))["all_remainder_wanted"] == 0
    assert sel(few(line_density=0.6))["all_remainder_wanted"] == 1
    assert sel(few(line_density=math.nextafter(0.6, 0.0)))["all_remainder_wanted"] == 0
    assert sel(few(rows=32_768, nnz=4_000_000))["all_remainder_wanted"] == 1
    assert sel(few(rows=32_767, nnz=4_000_000))["all_remainder_wanted"] == 0
    assert sel(few(nnz=3_999_999))["all_remainder_wanted"] == 0
    assert sel(few(cols=800_000))["all_remainder_wanted"] == 1
    assert sel(few(cols=799_999))["all_remainder_wanted"] == 0
    # a row's own window (xcd_gather_bytes less the columns' drift) must be beyond 3 MB
    assert sel(few(xcd_gather_bytes=5.0e6 + 3.0e6 + 8, nnz=15_000_000), tiled_min_rows=10_000_000)["all_remainder_wanted"] == 1
    assert sel(few(xcd_gather_bytes=5.0e6 + 3.0e6), tiled_min_rows=10_000_000)["all_remainder_wanted"] == 0
    assert sel(few(), no_pb_fallback=1)["all_remainder_wanted"] == 0
    assert sel(few(sharded=1))["all_remainder_wanted"] == 0
    # the second pass: any pattern, any row length, one row is enough
    d = sel(few(min_dense_override=0.0, sb_rows=512, longest_row=5000, n_long_rows=100_000, long_rows_nnz=10_000_000,
                whole=built(dense=0.0, nnz=15_000_000)))
    assert (d["min_rows"], d["min_dense"], d["kept"], d["form"]) == (1, 0.0, 1, "all-remainder")


def test_rule_8_thin_rows():
    """A piece-form copy of a matrix with under ten entries per row is dropped for the stream kernel."""
    r = 3_000_000
    assert sel(mid(nnz=10 * r, whole=built(pieces=512, nnz=10 * r)))["form"] == "pieces"
    d = sel(mid(nnz=10 * r - 1, tiling_share=0.5, whole=built(pieces=512, nnz=10 * r - 1)))
    assert (d["route"], d["kept"], d["note"], d["all_remainder_wanted"]) == (ROUTE["device_build"], 0, NOTE["thin"], 0)
    assert sel(big(nnz=8 * 5_000_000, whole=built(nnz=8 * 5_000_000)))["form"] == "fused"  # a fused copy keeps its thin rows


def test_rule_10_popular_far_entries():
    """A copy whose remainder (10 % of the entries or more) gathers to 80 % from 2 MB of popular columns while the window fits one
    L2 is dropped for the stream kernel."""
    f = big(xcd_gather_bytes=3.0e6, whole=built(dense=0.9, top=0.8))
    d = sel(f)
    assert (d["kept"], d["note"]) == (0, NOTE["popular"])
    assert sel(big(xcd_gather_bytes=3.0e6, whole=built(dense=0.9, top=math.nextafter(0.8, 0.0))))["kept"] == 1
    assert sel(big(xcd_gather_bytes=3.0e6, whole=dict(ok=1, n_pieces=0, dense_entries=90_000_001, n_rem=9_999_999, rem_top_share=0.9)))["kept"] == 1
    assert sel(big(xcd_gather_bytes=3.0e6 + 1, whole=built(dense=0.9, top=0.9)))["kept"] == 1
    assert sel(f, tiled_anyway=1)["kept"] == 1


def test_rule_11_few_rows_dense_tiles():
    """4-32 full-height super-blocks whose tiles would stage at most 1.8 vector bytes per entry byte go through the build."""
    rows, cols, nnz = 50_000, 2_000_000, 20_000_000

    def xcd_for(share):  # share = (span + 8192 cols / rows) * 8 / (nnz / rows * 8192 * 11), span = xcd / 8 - cols / 8
        span = share * (nnz / rows * SB * 11.0) / 8.0 - SB * cols / rows
        return 8.0 * span + cols

    f = dict(rows=rows, cols=cols, nnz=nnz, longest_row=500, line_density=0.9, sb_rows=SB, slots=SLOTS, whole=built(pieces=512, nnz=nnz),
             popular_share=0.05)
    d = sel(dict(f, xcd_gather_bytes=xcd_for(1.79)))
    assert (d["min_rows"], d["route"], d["form"]) == (rows, ROUTE["device_build"], "pieces")
    d = sel(dict(f, xcd_gather_bytes=xcd_for(1.81)))
    assert (d["min_rows"], d["route"], d["note"], d["all_remainder_wanted"]) == (32 * SB, ROUTE["few_rows"], NOTE["few_rows"], 1)
    assert sel(dict(f, rows=4 * SB, xcd_gather_bytes=xcd_for(0.5)))["route"] == ROUTE["device_build"]
    assert sel(dict(f, rows=4 * SB - 1, xcd_gather_bytes=xcd_for(0.5)))["route"] == ROUTE["few_rows"]
    assert sel(dict(f, nnz=3_999_999, xcd_gather_bytes=xcd_for(0.5)))["route"] == ROUTE["few_rows"]
    assert sel(dict(f, sb_rows=2048, xcd_gather_bytes=xcd_for(0.5)))["route"] == ROUTE["few_rows"]  # (a lowered height: 256 x 2048 rows)


def test_rule_12_thin_rows_before_the_build_and_with_long_rows_aside():
    r = 3_000_000
    thin = dict(nnz=10 * r - 1, whole=built(pieces=512, nnz=10 * r - 1))
    d = sel(mid(tiling_share=0.75, **thin))
    assert (d["route"], d["kept"], d["note"]) == (ROUTE["thin_early"], 0, NOTE["thin"])
    assert sel(mid(tiling_share=math.nextafter(0.75, 0.0), **thin))["route"] == ROUTE["device_build"]
    with pytest.raises(RuntimeError, match="tiling_share"):
        sel(mid(**thin))
    sel(mid())                                       # (ten or more per row: the test does not run)
    assert sel(mid(**thin), tiling_check=1)["route"] == ROUTE["device_build"]  # (hooks that want the build itself)
    assert sel(mid(**thin), host_tiling=1)["route"] == ROUTE["host_build"]
    long_rows = dict(longest_row=2000, n_long_rows=10, long_rows_nnz=20_000, popular_share=0.9, heaviest_pb_block=1)
    d = sel(mid(side=built(pieces=512), **long_rows))
    assert (d["route"], d["form"]) == (ROUTE["side_kept"], "pieces")
    d = sel(mid(tiling_share=0.5, side=built(pieces=512), **dict(long_rows, **thin)))
    assert (d["side_tried"], d["kept"], d["note"], d["long_rows_alone"]) == (1, 0, NOTE["shape"], 1)
    d = sel(mid(side=built(pieces=512, dense=0.74), **long_rows))
    assert (d["side_tried"], d["kept"], d["note"]) == (1, 0, NOTE["shape"])


def test_rule_13_long_rows_unpopular_columns():
    """Kept off the tiled forms for its long rows alone: all-remainder form where 32 768 popular lines take at most 30 % of the
    gathers and no 4096-row block holds more than 1 / 48 of the entries."""
    nnz = 48_000_000
    f = big(rows=400_000, nnz=nnz, longest_row=70_000, n_long_rows=5000, long_rows_nnz=12_000_000, xcd_gather_bytes=0.0, sb_rows=SB,
            popular_share=0.3, heaviest_pb_block=nnz // 48, tiled_min_rows_unused=0)
    f.pop("tiled_min_rows_unused")
    d = sel(f, tiled_min_rows=100_000)
    assert (d["note"], d["long_rows_alone"], d["all_remainder_wanted"]) == (NOTE["shape"], 1, 1)
    assert sel(dict(f, popular_share=math.nextafter(0.3, 1.0)), tiled_min_rows=100_000)["all_remainder_wanted"] == 0
    assert sel(dict(f, heaviest_pb_block=nnz // 48 + 1), tiled_min_rows=100_000)["all_remainder_wanted"] == 0
    assert sel(dict(f, line_density=0.59), tiled_min_rows=100_000)["all_remainder_wanted"] == 0
    assert sel(f, tiled_min_rows=100_000, no_pb_long_rows=1)["all_remainder_wanted"] == 0
    # skewed as well (rule 1 / the longest row): still for the row lengths alone
    d = sel(dict(f, long_row_share=0.4, n_long_rows=-1, long_rows_nnz=-1))
    assert (d["note"], d["long_rows_alone"], d["all_remainder_wanted"]) == (NOTE["skew"], 1, 1)
    # rows that share their lines are not such a candidate
    d = sel(dict(f, line_density=0.1, n_long_rows=-1, long_rows_nnz=-1))
    assert (d["note"], d["long_rows_alone"], d["all_remainder_wanted"]) == (NOTE["coalesced"], 0, 0)


def test_no_tiled_hook_leaves_the_stream_kernel_without_a_note():
    d = sel(big(), no_tiled=1)
    assert (d["route"], d["kept"], d["form"], d["note"], d["all_remainder_wanted"]) == (0, 0, "stream", "", 0)


def test_piece_form_expected_at_exactly_one_super_block_per_slot():
    """The three places that ask "will this copy run the piece form?" for a matrix of exactly `slots` full-height super-blocks:
    the one-L2 rule (4) counts it as fused (fewer super-blocks than slots = pieces), the imbalance rule (2) and the thin-rows
    tiling test (12) count it as pieces (at most as many)."""
    def at(nsb, **kw):
        rows = nsb * SB
        f = dict(rows=rows, cols=rows, nnz=20 * rows, longest_row=40, line_density=0.5, xcd_gather_bytes=3.0e6, sb_rows=SB, slots=SLOTS,
                 whole=built(pieces=512, nnz=20 * rows))
        f.update(kw)
        return f
    # rule 4
    assert sel(at(SLOTS - 1))["note"] == NOTE["one_l2"]
    assert sel(at(SLOTS))["route"] == ROUTE["device_build"]
    # rule 2: no block pass at exactly `slots` (the record above holds none), one from slots + 1 on
    sel(at(SLOTS, xcd_gather_bytes=8.0e6))
    with pytest.raises(RuntimeError, match="heaviest_block"):
        sel(at(SLOTS + 1, xcd_gather_bytes=8.0e6))
    # rule 12: the cheap tiling test runs at exactly `slots`, not beyond
    thin = dict(xcd_gather_bytes=8.0e6, line_density=0.9)
    with pytest.raises(RuntimeError, match="tiling_share"):
        sel(at(SLOTS, nnz=9 * SLOTS * SB, **thin))
    assert sel(at(SLOTS, nnz=9 * SLOTS * SB, tiling_share=0.8, **thin))["route"] == ROUTE["thin_early"]
    assert sel(at(SLOTS + 1, nnz=9 * (SLOTS + 1) * SB, heaviest_block=1, **thin))["route"] == ROUTE["device_build"]


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_covers_the_six_corpora():
    g = _golden()
    assert g["header"]["parent_commit"] and g["header"]["machine"]
    per = {}
    for r in g["records"]:
        per.setdefault(r["corpus"], set()).add(r["name"])
    assert {k: len(v) for k, v in per.items()} == {"tuning": 43, "held_out": 18, "held_out_2": 16, "boundaries": 16, "boundaries_2": 18,
                                                    "held_out_3": 8}
    assert len(g["records"]) == 2 * 119 and {r["matrix"] for r in g["records"]} == {"A", "A^T"}


def test_replay_of_the_corpus_gives_the_parents_forms_and_notes():
    bad = []
    for r in _golden()["records"]:
        passes = r["passes"]
        if not passes:  # (no pass ran)
            got = ("stream", "")
        else:
            d = sel(passes[0])
            if len(passes) == 2:
                if not d["all_remainder_wanted"] or d["kept"]:
                    bad.append((r["corpus"], r["name"], r["matrix"], "second pass without the first asking for it", d))
                    continue
                d = sel(passes[1])
            elif d["all_remainder_wanted"] and r["nnz"] > 4_000_000:  # (asked of matrices that went through the device transpose)
                bad.append((r["corpus"], r["name"], r["matrix"], "the first pass asks for a second that did not run", d))
                continue
            got = (d["form"], d["note"])
        if got != (r["parent_form"], r["parent_note"]):
            bad.append((r["corpus"], r["name"], r["matrix"], got, (r["parent_form"], r["parent_note"])))
    assert not bad, bad
