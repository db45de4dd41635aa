"""The BATCHED warm start BY VALUE in every panel geometry (GPU): kb_start_seed, kb_start_spmm<true|false> and kb_finalize of
hpr-lp-c_amd/csrc/batched.hip behind BatchedSolver.solve(..., X0, Y0) -- the seeded panels X, X_hat, X_bar, last_X and Y, Y_bar,
last_Y against the numpy projection of the host-scaled starts bit for bit, Z_bar and Y_obj per member against tests/startref.py's
high-precision reference ON THE SOLVER'S OWN READ-BACK panels, norms and scales within 2 x the derived bound of that module and
nothing wider, and primal_obj, gap and residuals per member likewise (residuals = the larger of err_Rp, err_Rd -- tests/evalref.py's
evaluator on the read-back panels -- and the start's gap).

A solve with max_iter = 0 runs ws_fill, ws_start (the three start kernels and their kb_finalize), one loop_evaluate(first = true)
(kb_resid<0>, kb_resid<1>, kb_lu, the fetch) and collect_results: loop_ended() gives every member ITER_LIMIT at iteration 0 before
any half-step runs (stop_tol = 1e-12 is out of reach of these starts; the module asserts status and iteration).

Geometries: those of tests/test_gpu_batched_ray_values.py (its docstring has the chunk widths): "long" with B = 1, 2, 3, 5, 12, 24,
64, 70, 130 and B = 70 with HPRLP_BATCH_CHUNK = 8, 16, 32; "short" with five; "mid" and "wrapped" at B = 64 -- "wrapped"
(8203 x 8209) is the only one in which kb_start_spmm's own row loop wraps.  The batches are tests/batched_ray_cases.py's: bound
kinds drawn per member and per line.  The starts: normal noise of scale 2 around the nearest finite bound (else 0) and of scale 1,
another seed per member, X0 = L resp. U exactly and Y0 = -0.0 on some lines; the second member of every chunk starts from zero and
the third has a zero Y0.  The first member of every chunk is also held against the reference with the dual completion leaning on
the wrong side, which must be out of tolerance.  With B = 70 the same data and starts go through solve_stream at width 8 (the
masked kb_start_* path): x, y, z of every problem are the bits of the plain batch just verified, and primal_obj, residuals and gap
those of the plain batch in chunks of 8, the geometry a stream of width 8 runs in -- the verified batch itself under
HPRLP_BATCH_CHUNK = 8, otherwise a second plain solve with the verified batch's x, y, z bits whose scalars are held to the same
references by value (the per-member sums are added in an order that follows the chunk width, so their bits differ between
geometries by design; measured: 49 of 70 primal_obj differ in the last place between chunks of 8 and of 16).

Largest observed-difference / bound ratio per quantity and geometry, MI355X (the tolerance is 2; the module prints the rows,
"LARGEST RATIOS"):

| geometry | Z_bar | Y_obj | primal_obj | gap | residuals |
|---|---|---|---|---|---|
| long B = 1 | 0.41 | 0.176 | 0.000257 | 0.000435 | 0.00153 |
| long B = 2 | 0.41 | 0.19 | 7.23e-05 | 0.000435 | 0.00769 |
| long B = 3 | 0.41 | 0.269 | 0.000355 | 0.000435 | 0.00987 |
| long B = 5 | 0.41 | 0.48 | 0.00153 | 0.00121 | 0.00987 |
| long B = 12 | 0.493 | 0.48 | 0.00236 | 0.00126 | 0.00987 |
| long B = 24 | 0.493 | 0.48 | 0.0027 | 0.00132 | 0.00987 |
| long B = 64 | 0.493 | 0.496 | 0.00485 | 0.00241 | 0.00987 |
| long B = 70 | 0.493 | 0.496 | 0.00699 | 0.00241 | 0.00987 |
| long B = 130 | 0.493 | 0.496 | 0.00699 | 0.00276 | 0.00987 |
| long B = 70, chunks of 8 | 0.493 | 0.496 | 0.00353 | 0.00221 | 0.00987 |
| long B = 70, chunks of 16 | 0.493 | 0.496 | 0.00353 | 0.0013 | 0.00987 |
| long B = 70, chunks of 32 | 0.493 | 0.496 | 0.00377 | 0.00279 | 0.00987 |
| short B = 3 | 0.386 | 0.246 | 0.000914 | 0.000104 | 0.0148 |
| short B = 12 | 0.418 | 0.438 | 0.00355 | 0.00148 | 0.0148 |
| short B = 64 | 0.485 | 0.438 | 0.00346 | 0.00161 | 0.0148 |
| short B = 70 | 0.485 | 0.438 | 0.00346 | 0.00161 | 0.0148 |
| short B = 70, chunks of 16 | 0.485 | 0.438 | 0.00452 | 0.00172 | 0.0148 |
| mid B = 64 | 0.474 | 0.559 | 0.000442 | 0.000607 | 0.00155 |
| wrapped B = 64 | 0.489 | 0.635 | 1.47e-05 | 4.25e-05 | 0.000144 |
| worst | 0.493 | 0.635 | 0.00699 | 0.00279 | 0.0148 |
"""
import numpy as np
import pytest

import batched_ray_cases as R
import evalref as E
import startref as S
from conftest import hprlp
from test_gpu_batched_ray_values import CASES, IDS, model_of

pytestmark = pytest.mark.gpu

DATA_PANELS = ("C", "AL", "AU", "L", "U")
SEEDED_N = ("X", "X_hat", "X_bar", "last_X")
SEEDED_M = ("Y", "Y_bar", "last_Y")
START_PANELS = SEEDED_N + SEEDED_M + ("Z_bar", "Y_obj")
NEW_PANELS = ("X", "X_hat", "last_X", "Y", "last_Y", "Z_bar", "Y_obj")
RESULT_FIELDS = ("x", "y", "z", "primal_obj", "residuals", "gap")
TABLE = ("Z_bar", "Y_obj", "primal_obj", "gap", "residuals")


def params():
    return hprlp.Parameters(max_iter=0, stop_tol=1e-12, check_iter=10, use_CR_scaling=False, use_presolve=False)


def starts(kind, B, Bw):
    """(X0, Y0, zero-start members, zero-Y0 members) in the caller's units"""
    s = R.shared(kind)
    m, n = s["m"], s["n"]
    inp = R.base_inputs(kind, B)
    L, U = inp["L"], inp["U"]
    X0, Y0 = np.zeros((n, B)), np.zeros((m, B))
    for k in range(B):
        rng = np.random.default_rng(R.member_seed(k, salt=40))
        centre = np.where(np.isfinite(L[:, k]), L[:, k], np.where(np.isfinite(U[:, k]), U[:, k], 0.0))
        X0[:, k] = centre + rng.normal(scale=2.0, size=n)
        Y0[:, k] = rng.normal(size=m)
    j, i = np.arange(n)[:, None], np.arange(m)[:, None]
    X0 = np.where((j % 16 == 3) & np.isfinite(L), L, np.where((j % 16 == 11) & np.isfinite(U), U, X0))
    Y0 = np.where(i % 16 == 5, -0.0, Y0)
    zero, zero_y = [k + 1 for k in range(0, B, Bw) if k + 1 < B], [k + 2 for k in range(0, B, Bw) if k + 2 < B]
    X0[:, zero] = 0.0
    Y0[:, zero] = 0.0
    Y0[:, zero_y] = 0.0
    return X0, Y0, zero, zero_y


def padding_is_zero(bs, name, rows, B, Bp, Bw):
    raw = bs.get_panel("raw:" + name).reshape(Bp // Bw, rows, Bw)
    pad = np.array([k >= B for k in range(Bp)]).reshape(Bp // Bw, 1, Bw)
    return raw.shape[0] * raw.shape[2] == Bp and not (raw * pad).any() and np.array_equal(raw[0, :, 0], bs.get_panel(name)[:, 0])


@pytest.mark.parametrize("kind,B,chunk,Bw", CASES, ids=IDS)
def test_batched_start_by_value_in_every_geometry(gpu, monkeypatch, kind, B, chunk, Bw):
    s = R.shared(kind)
    m, n, A, AT = s["m"], s["n"], s["A"], s["AT"]
    model = model_of(kind)
    bs = hprlp.BatchedSolver(model, params())
    base = R.base_inputs(kind, B)
    X0, Y0, zero, zero_y = starts(kind, B, Bw)
    tag = "%s B %d chunk %d" % (kind, B, chunk)
    if chunk:
        monkeypatch.setenv("HPRLP_BATCH_CHUNK", str(chunk))
    res = bs.solve(base["C"], base["AL"], base["AU"], base["L"], base["U"], X0=X0, Y0=Y0)
    info = bs.info()
    Bp = info["Bp"]
    assert (info["Bc"], Bp) == (Bw, 64 * -(-B // 64) if B > 64 else 1 << (B - 1).bit_length()), info
    assert res["status"] == ["ITER_LIMIT"] * B and not np.asarray(res["iter"]).any(), (tag, res["status"], res["iter"])
    norms = (bs.get_panel("row_norm"), bs.get_panel("col_norm"))
    assert np.array_equal(norms[0], s["row_norm"]) and np.array_equal(norms[1], s["col_norm"])
    scal = bs.scalars()

    # the new panels can be read and not written; the data panels with +-inf where the caller passed it
    got = {k: bs.get_panel(k) for k in DATA_PANELS + START_PANELS}
    for name in NEW_PANELS:
        with pytest.raises(RuntimeError, match="cannot be written"):
            bs.set_panel(name, got[name])
    panels = {k: got[k] for k in DATA_PANELS}
    for name in E.BOUND_PANELS:
        panels[name] = E.panel_bounds_to_inf(panels[name], base[name], name)

    # 1. the seeded panels: the projection of the host-scaled starts, bit for bit; the padding still zero
    prep = hprlp.batched_prepare_host(norms[0], norms[1], base["C"], base["AL"], base["AU"], base["L"], base["U"], X0, Y0)
    assert np.array_equal(prep["b_scale"], scal["b_scale"]) and np.array_equal(prep["c_scale"], scal["c_scale"]), tag
    assert np.array_equal(prep["X0"], (X0 * norms[1][:, None]) / scal["b_scale"]) and np.array_equal(prep["Y0"], (Y0 * norms[0][:, None]) / scal["c_scale"])
    Xs = np.minimum(np.maximum(prep["X0"], panels["L"]), panels["U"])
    Ys = np.where(np.isfinite(panels["AL"]), prep["Y0"], np.minimum(prep["Y0"], 0.0))
    Ys = np.where(np.isfinite(panels["AU"]), Ys, np.maximum(Ys, 0.0))
    for name in SEEDED_N:
        assert got[name].shape == (n, B) and np.array_equal(got[name], Xs), (tag, name, int((got[name] != Xs).sum()))
    for name in SEEDED_M:
        assert got[name].shape == (m, B) and np.array_equal(got[name], Ys), (tag, name, int((got[name] != Ys).sum()))
    assert (Xs != prep["X0"]).any() and (Ys != prep["Y0"]).any() and (Xs == prep["X0"]).any()
    assert (prep["X0"] < panels["L"]).any() and (prep["X0"] > panels["U"]).any()
    assert not Xs[:, zero][(panels["L"][:, zero] <= 0) & (panels["U"][:, zero] >= 0)].any() and not Ys[:, zero + zero_y].any()
    if Bp > B:
        for name in START_PANELS:
            assert padding_is_zero(bs, name, n if name in SEEDED_N + ("Z_bar",) else m, B, Bp, Bw), (tag, name, "padding")

    # 2. Z_bar, Y_obj and the results per member
    worst, refs = dict.fromkeys(TABLE, 0.0), []
    for k in range(B):
        inp = E.batched_member_inputs(A, AT, panels, norms, scal, k)
        xs, ys = got["X_bar"][:, k], got["Y_bar"][:, k]
        want = S.evaluate_start(*inp, xs, ys)
        label = "%s member %d" % (tag, k)
        r = S.check_vectors({"z_bar": got["Z_bar"][:, k], "y_obj": got["Y_obj"][:, k]}, want, label)
        st = dict(x_bar=xs, y_bar=ys, z_bar=got["Z_bar"][:, k], y_obj=got["Y_obj"][:, k], x_temp=np.zeros(n), y_temp=np.zeros(m),
                  last_x=xs, last_y=ys)
        sc4 = dict(inp[3], norm_b_org=float(scal["norm_b_org"][k]), norm_c_org=float(scal["norm_c_org"][k]))
        ev = E.evaluate(inp[0], inp[1], inp[2], sc4, st, 1.0, 1.0)
        assert ev["lu_term"][0] == 0, label
        kkt = (max(ev["err_Rd"][0], ev["err_Rp"][0], want["gap"][0]), max(ev["err_Rd"][1], ev["err_Rp"][1], want["gap"][1]))
        r = {"Z_bar": r["z_bar"], "Y_obj": r["y_obj"], "primal_obj": E.ratio(res["primal_obj"][k], want["primal_obj"]),
             "gap": E.ratio(res["gap"][k], want["gap"]), "residuals": E.ratio(res["residuals"][k], kkt)}
        assert E.all_within(r), (label, r, res["primal_obj"][k], res["gap"][k], res["residuals"][k], want["gap"], kkt)
        refs.append({"primal_obj": want["primal_obj"], "gap": want["gap"], "residuals": kkt})
        for name, v in r.items():
            worst[name] = max(worst[name], v)
        if k % Bw == 0:      # the first member of every chunk: the dual completion leaning on the wrong side is seen
            bad = S.evaluate_start(*inp, xs, ys, mutant="wrong-side")
            seen = (S.ratio(got["Z_bar"][:, k], bad["z_bar"]), E.ratio(res["gap"][k], bad["gap"]))
            assert min(seen) > S.TOL_FACTOR, (label, seen)
    assert (got["Z_bar"] > 0).any() and (got["Z_bar"] < 0).any() and (got["Z_bar"] == 0).any() and (got["Y_obj"] != 0).any()

    # 3. the results in the caller's units: the documented operations on the panels
    assert np.array_equal(res["x"], (got["X_bar"] / norms[1][:, None]) * scal["b_scale"]), tag
    assert np.array_equal(res["y"], (got["Y_bar"] / norms[0][:, None]) * scal["c_scale"]), tag
    assert np.array_equal(res["z"], (got["Z_bar"] * norms[1][:, None]) * scal["c_scale"]), tag

    # 4. the streamed call: the masked start kernels give every problem the plain batch's bits
    if B == 70:
        data = tuple(base[k] for k in DATA_PANELS)
        same = lambda a, b, f: np.array_equal(np.asarray(a[f]), np.asarray(b[f]))
        # x, y, z are elementwise maps of row sums in CSR order: the same bits in every geometry.  The per-member sums are added
        # up in an order that follows the chunk width (block_store_per_problem: 64 / Bc rows per wave), and a stream of width 8
        # runs in the geometry of a plain batch of 8 (Bc = 8): its scalars are held to the bits of the plain batch in chunks of 8
        # -- the batch just verified where that is its geometry, else a second plain solve whose x, y, z are the verified bits and
        # whose scalars are held to the same references by value.
        eight = res
        if Bw != 8:
            with monkeypatch.context() as mp:
                mp.setenv("HPRLP_BATCH_CHUNK", "8")
                b8 = hprlp.BatchedSolver(model, params())
                eight = b8.solve(*data, X0=X0, Y0=Y0)
                assert b8.info()["Bc"] == 8 and eight["status"] == res["status"]
                b8.close()
            assert all(same(eight, res, f) for f in ("x", "y", "z")), (tag, "chunks of 8")
            for k in range(B):
                r = {f: E.ratio(eight[f][k], refs[k][f]) for f in ("primal_obj", "gap", "residuals")}
                assert E.all_within(r), (tag, "chunks of 8, member %d" % k, r)
        out = bs.solve_stream(*data, width=8, X0=X0, Y0=Y0, prm=params())
        assert out["status"] == ["ITER_LIMIT"] * B and not np.asarray(out["iter"]).any(), tag
        assert bs.stream_info()["refills"] == B - 8 and bs.info()["Bc"] == 8, (bs.stream_info(), bs.info())
        for f in RESULT_FIELDS:
            against = res if f in ("x", "y", "z") else eight
            assert same(out, against, f), (tag, "stream", f, int((np.asarray(out[f]) != np.asarray(against[f])).sum()))
    print("batched start", tag, "LARGEST RATIOS", " | ".join("%s %.3g" % (k, worst[k]) for k in TABLE))
    bs.close(); model.free()
