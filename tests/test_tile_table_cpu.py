"""The shipped gfx950 tile table names only tiles the kernels know (host-side check; the GPU
suite, tests/test_tune_table_gpu.py, checks every entry's numerics on the device)."""
import json

from cxxnet_amd.ops import gemm as G


def _table():
    with open(G.TUNE_DB) as f:
        return json.load(f)


def test_every_entry_names_a_known_tile():
    bad = []
    for key, tile in _table().items():
        op = key.split("|")[0]
        if op == "cws":  # register weight-grad: tile * 100000 + K-split slices
            ok = tile // 100000 in G.TILES and tile % 100000 >= 1
        elif op in ("cf", "cd"):  # also the direct small-map kernel's schedules (conv_direct.hip)
            ok = tile in G.GLDS_TILES or tile == G.REG or tile in G.DIRECT_TILES
        elif op in ("cw", "cfs"):
            ok = tile in G.GLDS_TILES or tile == G.REG
        else:  # cr, cwr, fc, fw, fws: LDS-DMA tiles only
            ok = tile in G.GLDS_TILES
        if not ok:
            bad.append((key, tile))
    assert not bad, bad[:10]


def test_tuning_candidates_are_known_tiles():
    assert set(G.GLDS_CANDS) <= set(G.GLDS_TILES)
    for t in (82, 114, 130, 131, 133):  # wave-quantisation (r3), one-wave-per-SIMD, halo (r4)
        assert t in G.GLDS_CANDS


def _compiled_tiles():
    """Tile ids the kernels' dispatch code accepts, read from the HIP sources."""
    import os
    import re
    kdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(G.__file__))), "csrc", "kernels")
    src = lambda f: open(os.path.join(kdir, f)).read()
    tiles = set()
    glds = src("gemm_glds.hip")
    body = glds[glds.index("#define CXG_KK_TILES"):glds.index("#define CXG_CASE")]
    tiles |= {int(m) for m in re.findall(r"CXG_T[PC]?\((\d+),", body)}
    tiles |= {int(m) for m in re.findall(r"case (\d+): launch_4f", src("gemm_4w.hip"))}
    halo = src("conv_halo.hip")
    tiles |= {int(m) for m in re.findall(r"tile == (\d+)", halo[halo.index("int dispatch_halo"):])}
    wg = src("conv_wgrad_halo.hip")
    tiles |= {int(m) for m in re.findall(r"tile [!=]= (\d+)", wg[wg.index("int dispatch_wgrad_halo"):])}
    return tiles


def test_tile_dict_matches_compiled_kernels():
    """Every tile the Python side can name is compiled, and no compiled tile is orphaned."""
    compiled = _compiled_tiles()
    assert set(G.GLDS_TILES) == compiled, (sorted(set(G.GLDS_TILES) - compiled), sorted(compiled - set(G.GLDS_TILES)))


def test_every_compiled_tile_is_used():
    """A compiled tile is in the shipped table, a default pick, or the fc weight-grad set."""
    used = {t for k, t in _table().items() if k.split("|")[0] != "cws"}
    used |= {1, 7, 10, 15}  # _pick_glds defaults
    used |= {141, 142}  # forced patch widths of the 140 kernel (same template instances)
    used |= {82}  # 256x192 wave-quantisation tile: a step_tune candidate (AlexNet conv3 data-grad moved to the direct kernel)
    unused = sorted(_compiled_tiles() - used)
    assert not unused, unused


def test_signature_keys_are_well_formed():
    for key in _table():
        parts = key.split("|")
        assert parts[0] in G.SIG_FIELDS, key
        assert len(parts) - 1 == len(G.SIG_FIELDS[parts[0]]), key
        assert all(p.lstrip("-").isdigit() for p in parts[1:]), key
        assert G.sig(parts[0], *[int(p) for p in parts[1:]]) == key


# ------------------------------------------------------------------------------- served matrix
def _kernel_src(name):
    import os
    kdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(G.__file__))), "csrc", "kernels")
    with open(os.path.join(kdir, name)) as f:
        return f.read()


def glds_served_matrix():
    """(KK tile ids, MM tile ids, {(amode, bmode, epilogue): "KK" | "MM"}) of dispatch() in
    gemm_glds.hip: which tile set each compiled operand / epilogue form accepts."""
    import re
    glds = _kernel_src("gemm_glds.hip")
    kk = glds[glds.index("#define CXG_KK_TILES"):glds.index("#define CXG_MM_TILES")]
    mm = glds[glds.index("#define CXG_MM_TILES"):glds.index("#define CXG_CASE")]
    ids = lambda body: {int(m) for m in re.findall(r"CXG_T[PC]?\((\d+),", body)}  # noqa: E731
    forms = {(a, b, e): t for a, b, e, t in
             re.findall(r"^\s*CXG_CASE\((\w+), (\w+), (\w+), CXG_(KK|MM)_TILES\)", glds, re.M)}
    return ids(kk), ids(mm), forms


# the form(s) each op class of the table launches (ops/gemm.py); every form of a class must
# take the same tile set for the table below to hold
OP_FORMS = {
    "cf": [("K_DIRECT", "K_GATHER", "EPI_BF16")],
    "cd": [("K_DIRECT", "K_GATHER", "EPI_BF16"), ("K_DIRECT", "K_GATHER", "EPI_BF16_DB"),
           ("K_DIRECT", "K_GATHER", "EPI_BF16_ADD")],
    "cfs": [("K_DIRECT", "K_GATHER", "EPI_BF16")],
    "cr": [("K_DIRECT", "K_ROWGATHER", "EPI_BF16")],
    "fc": [("K_DIRECT", "K_DIRECT", "EPI_BF16"), ("K_DIRECT", "K_DIRECT", "EPI_F32")],
    "cw": [("MN_GATHER", "MN_DIRECT", "EPI_F32_ATOMIC")],
    "cwr": [("MN_GATHER", "MN_DIRECT", "EPI_F32_ATOMIC")],
    "fw": [("MN_DIRECT", "MN_DIRECT", "EPI_F32"), ("MN_DIRECT", "MN_DIRECT", "EPI_F32_ACC")],
    "fws": [("MN_DIRECT", "MN_DIRECT", "EPI_F32_SGD")],
}
# ids outside gemm_glds.hip's switches that an op class may also hold: the register kernel, the
# one-wave-per-SIMD tile, the halo kernels and the direct kernel's schedules
ALSO = {"cf": {G.REG, 114, 130, 131, 132, 133} | set(G.DIRECT_TILES),  # (132 is retired: not a known tile)
        "cd": {G.REG, 114, 130, 131, 132, 133} | set(G.DIRECT_TILES),
        "cw": {G.REG, 140, 141, 142}}
# table entries left on a tile their form does not compile (a fallback kernel runs them), each
# with the measurement that kept it.  None: the two fc forward entries that named the MN-major
# tile 2 were re-timed against every K-major tile and the register kernel they fell back to.
KNOWN_DECLINED = set()


def served_tiles(op):
    kk, mm, forms = glds_served_matrix()
    sets = {forms[f] for f in OP_FORMS[op]}
    assert len(sets) == 1, (op, sets)
    return (kk if sets == {"KK"} else mm) | ALSO.get(op, set())


def test_dispatch_forms_are_the_ones_the_ops_launch():
    kk, mm, forms = glds_served_matrix()
    assert kk == {1, 7, 10, 15, 21, 25, 30, 31, 34, 37, 38, 39, 72, 75, 76, 77, 78, 79, 82}
    assert mm == {1, 2, 17, 23, 40, 41}
    assert set(forms) == {f for fs in OP_FORMS.values() for f in fs}
    for op in OP_FORMS:
        served_tiles(op)


def _4w_fast_ok(op, f):
    """fast_ok of gemm_4w.hip for the gather operand of a cf / cd entry: Cg % 64, kdim % 64, at
    most 32 taps (cd: the gathered tensor is dy, Cg = cg_out)."""
    g = dict(zip(G.SIG_FIELDS[op], f))
    cg = (g["C"] if op == "cf" else g["Cout"]) // g["groups"]
    taps = g["KH"] * g["KW"]
    return cg % 64 == 0 and (taps * cg) % 64 == 0 and taps <= 32 and (op == "cf" or g["stride"] == 1)


def test_every_entry_names_a_tile_its_form_compiles():
    """A table entry whose tile the op's form does not compile is not an error at run time: the
    dispatch returns -1 and a fallback kernel runs the layer silently.  Every entry must name a
    tile that serves its op class (or be listed, with the reason, in KNOWN_DECLINED)."""
    bad = []
    for key, tile in _table().items():
        parts = key.split("|")
        op = parts[0]
        if op == "cws":
            continue  # register-kernel ids, checked in test_every_entry_names_a_known_tile
        ok = tile in served_tiles(op)
        if ok and tile == 114:
            ok = _4w_fast_ok(op, [int(p) for p in parts[1:]])
        if not ok and key not in KNOWN_DECLINED:
            bad.append((key, tile))
    assert not bad, bad
    stale = [k for k in KNOWN_DECLINED if k not in _table() or _table()[k] in served_tiles(k.split("|")[0])]
    assert not stale, stale
