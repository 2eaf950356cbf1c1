"""CPU-only checks of the C-ABI library: it loads, exports every symbol include/msi_hip.h
declares, its host-side entry points (trig tables, layer table, weight packing) agree with the
oracle / with an index-level restatement, and argument errors come back as codes, not crashes.
No kernel is launched here (there is no GPU in the build container)."""
import os
import re

import numpy as np
import pytest

from oracle import geometry as G
from oracle import nets as onets
from tests.util import check_binding, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_header_symbol_is_exported(native_lib):
    declared = set(re.findall(r"\b(msi_[a-z0-9_]+)\s*\(", header_text()))
    assert len(declared) >= 17
    assert declared == set(native_lib.SIGNATURES), declared ^ set(native_lib.SIGNATURES)
    for name in declared:
        assert hasattr(native_lib.lib, name), name
    assert native_lib.lib.msi_version().startswith(b"msi_hip")


def _signature_names():
    """(collection time: the names from the binding's source text, not from an import of it, which needs the built library)"""
    text = open(os.path.join(ROOT, "matryodshka_amd", "_native.py")).read()
    return re.findall(r'^    "(msi_[a-z0-9_]+)": \(', text[text.index("SIGNATURES = {"):], flags=re.M)


def test_the_signature_test_covers_every_binding(native_lib):
    assert sorted(_signature_names()) == sorted(native_lib.SIGNATURES) and len(_signature_names()) >= 60


@pytest.mark.parametrize("name", _signature_names())
def test_header_and_binding_agree_on_every_signature(native_lib, name):
    """The return type and every parameter of _native.SIGNATURES[name] against the header's declaration (tests.util.declared): a
    scalar as its ctype, a pointer as the typed pointer or as c_void_p."""
    check_binding(native_lib, name)


def test_library_has_no_high_half_to_low_lane_packed_operand(native_lib):
    """matryodshka_amd/isa_lint.py (r05, DESIGN.md section 4 "the wobble"): no packed-fp32 VALU instruction of the linked library routes the HIGH
    half of a register pair to its LOW lane -- the compiler-made form whose low product came out 0 for 16 lanes in ~0.1 % of forwards.  The lint
    must also recognise the form (checked on the instruction that failed, as llvm-objdump prints it)."""
    from matryodshka_amd import isa_lint
    assert isa_lint.FORBIDDEN.match("\tv_pk_mul_f32 v[46:47], v[18:19], v[50:51] op_sel:[0,1] op_sel_hi:[1,0]")
    assert isa_lint.FORBIDDEN.match("\tv_pk_add_f32 v[18:19], v[46:47], v[18:19] op_sel:[1,0] op_sel_hi:[0,1]")
    assert not isa_lint.FORBIDDEN.match("\tv_pk_add_f32 v[24:25], v[14:15], s[50:51] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]")
    assert not isa_lint.FORBIDDEN.match("\tv_pk_fma_f32 v[16:17], v[80:81], s[4:5], v[64:65] op_sel_hi:[1,0,1]")
    objs = isa_lint.code_objects(native_lib.LIB_PATH)
    assert len(objs) >= 2 and all("gfx950" in t for t, _ in objs), [t for t, _ in objs]
    assert isa_lint.lint(native_lib.LIB_PATH) == []


def test_lint_recognises_a_valu_write_of_a_wide_stores_data_in_the_next_instruction():
    """matryodshka_amd/isa_lint.py, second rule (r05, DESIGN.md section 4 "the lost stores"): `buffer_store_dwordx4 vdata, ..., sN offen` followed at once by a VALU
    write of vdata lost a few stores per launch on gfx950 -- hipcc inserts the wait state only when soffset is not a register.  The parsers, on the instructions of
    the build that failed (the library itself is checked by the test above)."""
    from matryodshka_amd import isa_lint
    assert isa_lint._store_data("\tbuffer_store_dwordx4 v[46:49], v86, s[8:11], s14 offen") == (46, 49)
    assert isa_lint._store_data("\tbuffer_store_dwordx3 v[4:6], v1, s[0:3], 0 offen offset:16") == (4, 6)
    assert isa_lint._store_data("\tglobal_store_dwordx4 v[2:3], v[10:13], off") == (10, 13)        # (global / flat: the address comes first)
    assert isa_lint._store_data("\tglobal_store_dwordx4 v8, v[10:13], s[4:5] offset:32") == (10, 13)
    assert isa_lint._store_data("\tbuffer_store_dwordx2 v[46:47], v86, s[8:11], s14 offen") is None  # (64 bits: no hazard)
    assert isa_lint._store_data("\tbuffer_load_dwordx4 v[46:49], v86, s[8:11], s14 offen") is None
    assert isa_lint._valu_dest("\tv_mul_lo_u32 v46, v98, s28") == (46, 46)
    assert isa_lint._valu_dest("\tv_mad_u64_u32 v[86:87], s[4:5], v86, s14, v[94:95]") == (86, 87)
    assert isa_lint._valu_dest("\tv_cmp_eq_u32_e32 vcc, s15, v46") is None
    assert isa_lint._valu_dest("\tv_readfirstlane_b32 s15, v46") is None
    assert isa_lint._valu_dest("\ts_mov_b64 s[28:29], exec") is None


def test_lint_tracks_every_pending_store_and_every_vgpr_a_valu_instruction_writes():
    """Round 6 (ADVICE r05 / VERDICT r05 item 5d): back-to-back stores each keep their own wait-state count; v_swap_b32 writes both operands; MFMA / 64-bit
    destinations are ranges; load destinations on a just-stored register are counted, not refused (the module docstring says why)."""
    from matryodshka_amd import isa_lint
    scan = isa_lint.scan_kernel_text
    a = "\tbuffer_store_dwordx4 v[46:49], v86, s[8:11], 0 offen"
    b = "\tbuffer_store_dwordx4 v[50:53], v86, s[8:11], 0 offen offset:16"
    # store A; store B; VALU write of A's data: one wait state behind A (the r05 lint forgot A when it saw B)
    bad, nstore, nload = scan([a, b, "\tv_mul_lo_u32 v46, v98, s28"])
    assert nstore == 2 and len(bad) == 1 and "v[46:49]" in bad[0] and "(1 wait state(s))" in bad[0]
    # ... and of B's data, zero wait states behind B
    bad, _, _ = scan([a, b, "\tv_add_u32 v53, v1, v2"])
    assert len(bad) == 1 and "v[50:53]" in bad[0] and "(0 wait state(s))" in bad[0]
    # two wait states behind A (an s_nop 0 counts one; s_nop 1 two): clean
    assert scan([a, "\ts_nop 0", "\tv_mov_b32 v5, v6", "\tv_mul_lo_u32 v46, v98, s28"])[0] == []
    assert scan([a, "\ts_nop 1", "\tv_mul_lo_u32 v46, v98, s28"])[0] == []
    assert len(scan([a, "\ts_nop 0", "\tv_mul_lo_u32 v46, v98, s28"])[0]) == 1
    # v_swap_b32 writes BOTH operands
    assert len(scan([a, "\tv_swap_b32 v3, v47"])[0]) == 1
    assert isa_lint.vgpr_writes("\tv_swap_b32 v3, v47") == [((3, 3), "valu"), ((47, 47), "valu")]
    # MFMA / accvgpr reads: the whole destination range
    assert isa_lint.vgpr_writes("\tv_mfma_f32_32x32x16_bf16 v[40:55], v[2:5], v[6:9], v[40:55]") == [((40, 55), "valu")]
    assert len(scan([a, "\tv_mfma_f32_32x32x16_bf16 v[40:55], v[2:5], v[6:9], v[40:55]"])[0]) == 1
    assert isa_lint.vgpr_writes("\tv_accvgpr_read_b32 v48, a3") == [((48, 48), "valu")]
    assert isa_lint.vgpr_writes("\tv_accvgpr_write_b32 a3, v48") == []
    # loads: recognised, counted, not refused; LDS-DMA loads have no VGPR destination
    assert isa_lint.vgpr_writes("\tglobal_load_dwordx4 v[14:17], v[2:3], off offset:32") == [((14, 17), "load")]
    assert isa_lint.vgpr_writes("\tds_read_b128 v[116:119], v26") == [((116, 119), "load")]
    assert isa_lint.vgpr_writes("\tbuffer_load_dwordx4 v1, s[8:11], s14 offen lds") == []
    bad, _, nload = scan(["\tglobal_store_dwordx4 v[10:11], v[14:17], off", "\tglobal_load_dwordx4 v[14:17], v[2:3], off offset:32"])
    assert bad == [] and nload == 1
    assert isa_lint._find_objdump().endswith("llvm-objdump")


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under matryodshka_amd/ or include/ may mention it."""
    for base in ("matryodshka_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".cpp", ".h")):
                    text = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), os.path.join(dirpath, f)


@pytest.mark.parametrize("h,w", [(320, 640), (32, 64), (640, 1280), (20, 50)])
def test_trig_tables_bit_equal_oracle(native_lib, h, w):
    n = native_lib.lib.msi_trig_table_floats(h, w)
    assert n == 2 * w + 2 * h
    tab = np.empty(n, np.float32)
    assert native_lib.lib.msi_build_trig_tables_host(h, w, tab.ctypes.data) == 0
    cs, ss, ct, st = G.trig_tables(h, w)
    assert np.array_equal(tab[:w], cs) and np.array_equal(tab[w:2 * w], ss)
    assert np.array_equal(tab[2 * w:2 * w + h], ct) and np.array_equal(tab[2 * w + h:], st)


def test_bad_arguments_return_codes(native_lib):
    lib = native_lib.lib
    assert lib.msi_build_trig_tables_host(0, 8, None) == -1
    assert b"bad arguments" in lib.msi_last_error_string()
    assert lib.msi_ods_sphere_sweep_f32(None, None, None, None, None, 1, 8, 8, 4, 1, None, 24, 0, None) == -1
    assert lib.msi_compose_poses_f32(None, None, None, 1, None) == -1
    assert lib.msi_render_equirect_f32(None, None, None, None, None, 1, 8, 8, 4, None, None, None, None) == -1
    assert lib.msi_assemble_rgba_f32(None, None, None, None, None, 1, 8, 8, 4, None) == -1
    from matryodshka_amd import nets
    bad = nets.make_desc(1, 30, 64, 24, 8, 16, True)        # height not a multiple of 8
    assert lib.msi_net_workspace_bytes(bad) == 0 and b"multiples of 8" in lib.msi_last_error_string()


def test_variable_table_matches_oracle_and_reference_count(native_lib):
    from matryodshka_amd import nets
    for coord in (True, False):
        shapes = dict(nets.variable_shapes(192, 64, 64, coord))
        ow = onets.init_weights(192, 64, 64, coord)
        assert {k: tuple(v.shape) for k, v in ow.items()} == {k: tuple(v) for k, v in shapes.items()}
    desc = nets.make_desc(1, 320, 640, 192, 64, 64, True)
    assert native_lib.lib.msi_net_param_floats(desc) == 16980160
    infos = nets.layer_infos(desc)
    assert [i.name.decode() for i in infos] == nets.LAYER_NAMES
    assert (infos[0].out_h, infos[0].out_w, infos[9].out_h, infos[9].out_w) == (320, 640, 40, 80)
    assert (infos[10].kind, infos[10].cin, infos[10].cout, infos[10].out_h) == (1, 1024, 256, 80)
    blob = nets.flatten_params(ow if coord else ow, 192, 64, 64, False)
    back = nets.unflatten_params(blob, 192, 64, 64, False)
    assert all(np.array_equal(back[k], ow[k]) for k in ow)


def _unswizzle_row(row, n, dtype="f32"):
    """Packed rows store data chunk j^((n>>1)&7) in 16-byte slot j (bank-conflict-free LDS image).
    `row` is the 128-byte row as 32 float32 words; bf16 rows come back as 64 fp32 values."""
    swz = (n >> 1) & 7
    out = np.empty_like(row)
    for j in range(8):
        out[(j ^ swz) * 4:(j ^ swz) * 4 + 4] = row[j * 4:j * 4 + 4]
    if dtype == "bf16":
        return (out.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("coord", [True, False])
def test_weight_packing_index_level(native_lib, coord, dtype):
    """msi_net_pack_weights_host against an index-level restatement of the documented layout
    [class][k-step][npad][128 bytes]: k-steps are tap-major, then source-0 chunks, then source-1 chunks.
    A row holds 32 fp32 or 64 bf16 (round to nearest even) channels.  The CoordNet channel is not a k-step:
    its contribution is the fp32 table [out_row][5 column classes][Cout] behind gamma / beta."""
    from matryodshka_amd import nets
    cin, nout, ngf = 24, 8, 16
    same_pad = bool(coord)      # msi_coord_train_net pads SAME; msi_train_net wrap-pads and runs VALID
    bke = 64 if dtype == "bf16" else 32
    w = onets.init_weights(cin, nout, ngf, coord, seed=3, randomize_affine=True)
    desc = nets.make_desc(1, 16, 32, cin, nout, ngf, coord, dtype=dtype)
    packed = nets.pack_params(desc, nets.flatten_params(w, cin, nout, ngf, coord))
    rnd = onets.bf16_round if dtype == "bf16" else (lambda a: a)
    infos = nets.layer_infos(desc)
    off = 0
    skips = {"conv6_1": (ngf * 8, ngf * 8), "conv7_1": (ngf * 4, ngf * 4), "conv8_1": (ngf * 2, ngf * 2)}
    for info in infos:
        name = info.name.decode()
        wt = w[name + "/weights"]
        c0, c1 = skips.get(name, (info.cin, 0))
        cpt0, cpt1 = -(-c0 // bke), -(-c1 // bke)
        ntaps = {0: 9, 1: 4, 2: 1}[info.kind]
        ncls = 4 if info.kind == 1 else 1
        ksteps = ntaps * (cpt0 + cpt1)
        npad = -(-info.cout // 128) * 128
        wp = packed[off:off + ncls * ksteps * npad * 32].reshape(ncls, ksteps, npad, 32)
        rng = np.random.RandomState(hash(name) % 1000)
        for _ in range(40):
            cls, s, n = rng.randint(ncls), rng.randint(ksteps), rng.randint(info.cout)
            row = _unswizzle_row(wp[cls, s, n], n, dtype)
            exp = np.zeros(bke, np.float32)
            if True:
                tap, within = divmod(s, cpt0 + cpt1)
                src, chunk = (0, within) if within < cpt0 else (1, within - cpt0)
                base, csrc = (0, c0) if src == 0 else (c0, c1)
                for kk in range(bke):
                    if chunk * bke + kk >= csrc:
                        continue
                    c = base + chunk * bke + kk
                    if info.kind == 0:
                        exp[kk] = wt[tap // 3, tap % 3, c, n]
                    elif info.kind == 1:
                        ph, pw = cls >> 1, cls & 1
                        th, tw = tap >> 1, tap & 1
                        if same_pad:    # SAME: y[2i+k-1] += x[i] w[k]
                            kh = 1 + 2 * th if ph == 0 else 2 - 2 * th
                            kw = 1 + 2 * tw if pw == 0 else 2 - 2 * tw
                        else:        # VALID over wrap_pad(x, 2, 2) (uncropped output): k = parity + 2 * tap
                            kh, kw = ph + 2 * th, pw + 2 * tw
                        exp[kk] = wt[kh, kw, n, c]
                    else:
                        exp[kk] = wt[0, 0, c, n]
            assert np.array_equal(row, rnd(exp)), (name, cls, s, n)
        assert not wp[:, :, info.cout:, :].any()          # N padding is zero
        off_next = off + wp.size
        # gamma/beta (or bias) follow the weights
        if info.kind == 2:
            assert np.array_equal(packed[off_next:off_next + info.cout], w[name + "/biases"])
        else:
            assert np.array_equal(packed[off_next:off_next + info.cout], w[name + "/LayerNorm/gamma"])
        # next layer's packed offset: walk by the library's own rule (64-float alignment)
        r4 = -(-info.cout // 4) * 4
        off = off_next + 2 * r4
        # the fixed-point window of the layer's LayerNorm sums: four doubles {S1, S2, 1/S1, 1/S2} = 2^(24 - e), 2^(16 - 2e)
        # and their inverses, e from the weights (exact powers of two, consistent with each other)
        scl = packed[off:off + 8].view(np.float64)
        if info.kind != nets.KIND_HEAD:
            e = 24 - int(np.log2(scl[0]))
            assert scl[0] == 2.0 ** (24 - e) and scl[1] == 2.0 ** (16 - 2 * e) and scl[2] == 1.0 / scl[0] and scl[3] == 1.0 / scl[1]
            assert -8 <= e <= 8, (name, e)         # Xavier weights, unit gamma: raw outputs of order one
        else:
            assert not scl.any()
        off += 8
        if info.has_coord:
            # CoordNet bias table: sum over the in-image taps of coord[ih] * w[kh, kw, cin, n]
            tab = packed[off:off + info.out_h * 5 * r4].reshape(info.out_h, 5, r4)
            coord = rnd(np.abs(np.sin(np.linspace(-np.pi / 2.0, np.pi / 2.0, info.in_h))).astype(np.float32)).astype(np.float64)
            wc = rnd(wt[:, :, info.cin, :]).astype(np.float64)                     # [3,3,Cout]
            keff = 2 * info.rate + 1
            pad_t = max((info.out_h - 1) * info.stride + keff - info.in_h, 0) // 2
            pad_l = max((info.out_w - 1) * info.stride + keff - info.in_w, 0) // 2
            reps = [0, 1, 2, info.out_w - 2, info.out_w - 1]
            for mh in (0, 1, info.out_h // 2, info.out_h - 1):
                for cc, mw in enumerate(reps):
                    exp = np.zeros(info.cout)
                    for kh in range(3):
                        for kw in range(3):
                            ih, iw = mh * info.stride - pad_t + kh * info.rate, mw * info.stride - pad_l + kw * info.rate
                            if 0 <= ih < info.in_h and 0 <= iw < info.in_w:
                                exp += coord[ih] * wc[kh, kw]
                    assert np.allclose(tab[mh, cc, :info.cout], exp, rtol=1e-6, atol=1e-7), (name, mh, cc)
            off += tab.size
        off = -(-off // 64) * 64
        # fp32 plans: the x3 block (plan option F32_SPLIT3) of a one-source 3x3 layer or a SAME conv-transpose whose sources are whole
        # 32-channel chunks: the same k-steps as above, each as three planes of 64-byte rows -- [class][k-step][plane h | m | l][npad][32 bf16];
        # h = bf16(w), m = bf16(w - h), l = bf16(w - h - m); 16-byte slot j of row n stored at j ^ ((n >> 2) & 3)
        if dtype == "f32" and ((info.kind == 0 and c1 == 0 and c0 % 32 == 0) or (info.kind == 1 and c0 % 32 == 0 and c1 % 32 == 0)):
            blk = packed[off:off + ncls * ksteps * 3 * npad * 16].view(np.uint16).reshape(ncls, ksteps, 3, npad, 32)
            for _ in range(40):
                cls, s_, n = rng.randint(ncls), rng.randint(ksteps), rng.randint(info.cout)
                tap, within = divmod(s_, cpt0 + cpt1)
                src, chunk = (0, within) if within < cpt0 else (1, within - cpt0)
                cb = (0 if src == 0 else c0) + chunk * 32
                if info.kind == 0:
                    want = wt[tap // 3, tap % 3, cb:cb + 32, n].astype(np.float32)
                else:
                    ph, pw = cls >> 1, cls & 1
                    th, tw = tap >> 1, tap & 1
                    if same_pad:
                        kh = 1 + 2 * th if ph == 0 else 2 - 2 * th
                        kw = 1 + 2 * tw if pw == 0 else 2 - 2 * tw
                    else:        # VALID over wrap_pad(x, 2, 2): k = parity + 2 * tap
                        kh, kw = ph + 2 * th, pw + 2 * tw
                    want = wt[kh, kw, n, cb:cb + 32].astype(np.float32)
                parts = []
                for pl in range(3):
                    row = blk[cls, s_, pl, n].reshape(4, 8)
                    un = np.empty_like(row)
                    for j in range(4):
                        un[j ^ ((n >> 2) & 3)] = row[j]
                    parts.append((un.reshape(32).astype(np.uint32) << 16).view(np.float32))
                h = onets.bf16_round(want)
                m = onets.bf16_round(want - h)
                l = onets.bf16_round(want - h - m)
                assert np.array_equal(parts[0], h) and np.array_equal(parts[1], m) and np.array_equal(parts[2], l), (name, cls, s_, n)
                assert np.abs((parts[0].astype(np.float64) + parts[1] + parts[2]) - want).max() <= 2.0 ** -24 * np.abs(want).max()
            assert not blk[:, :, :, info.cout:, :].any()
            off = -(-(off + blk.size // 2) // 64) * 64
            # ... followed by the x2 block (plan option F32_SPLIT_F16): the same rows as TWO fp16 planes, h = fp16(w) and
            # m' = fp16((w - h) 2^11) -- w = h + m' 2^-11 to 22 significand bits
            blk2 = packed[off:off + ncls * ksteps * 2 * npad * 16].view(np.float16).reshape(ncls, ksteps, 2, npad, 32)
            for _ in range(40):
                cls, s_, n = rng.randint(ncls), rng.randint(ksteps), rng.randint(info.cout)
                tap, within = divmod(s_, cpt0 + cpt1)
                src, chunk = (0, within) if within < cpt0 else (1, within - cpt0)
                cb = (0 if src == 0 else c0) + chunk * 32
                if info.kind == 0:
                    want = wt[tap // 3, tap % 3, cb:cb + 32, n].astype(np.float32)
                else:
                    ph, pw = cls >> 1, cls & 1
                    th, tw = tap >> 1, tap & 1
                    if same_pad:
                        kh = 1 + 2 * th if ph == 0 else 2 - 2 * th
                        kw = 1 + 2 * tw if pw == 0 else 2 - 2 * tw
                    else:        # VALID over wrap_pad(x, 2, 2): k = parity + 2 * tap
                        kh, kw = ph + 2 * th, pw + 2 * tw
                    want = wt[kh, kw, n, cb:cb + 32].astype(np.float32)
                parts = []
                for pl in range(2):
                    row = blk2[cls, s_, pl, n].reshape(4, 8)
                    un = np.empty_like(row)
                    for j in range(4):
                        un[j ^ ((n >> 2) & 3)] = row[j]
                    parts.append(un.reshape(32))
                h = want.astype(np.float16)
                m = ((want - h.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
                assert np.array_equal(parts[0], h) and np.array_equal(parts[1], m), (name, cls, s_, n)
                assert np.abs(parts[0].astype(np.float64) + parts[1].astype(np.float64) / 2048.0 - want).max() <= 2.0 ** -21 * np.abs(want).max()
            assert not blk2[:, :, :, info.cout:, :].any()
            off = -(-(off + blk2.size // 2) // 64) * 64
    if dtype == "bf16":
        # bf16 plans end with the head's bf16-ROUNDED weights once more as fp32 rows (32 channels per 128-byte row, rows
        # padded to 64, slots swizzled like every fp32 row): the fused tail runs the 1x1 head on the fp32 MFMA
        head = infos[-1]
        wt = w[head.name.decode() + "/weights"]
        ks32, npad32 = -(-head.cin // 32), -(-head.cout // 64) * 64
        hp = packed[off:off + ks32 * npad32 * 32].reshape(ks32, npad32, 32)
        for ks in range(ks32):
            for n in range(head.cout):
                exp = np.zeros(32, np.float32)
                m = min(32, head.cin - ks * 32)
                exp[:m] = onets.bf16_round(wt[0, 0, ks * 32:ks * 32 + m, n])
                assert np.array_equal(_unswizzle_row(hp[ks, n], n, "f32"), exp), (ks, n)
        assert not hp[:, head.cout:, :].any()
        off = -(-(off + hp.size) // 64) * 64
    assert off == packed.size


def test_plan_layer_params_reports_its_size_and_checks_its_arguments(native_lib):
    import ctypes
    from matryodshka_amd import nets
    N = native_lib
    plan = N.NetPlan(nets.make_desc(1, 64, 128, 96, 32, 64, True))
    need = ctypes.c_size_t(0)
    assert N.lib.msi_net_plan_layer_params(plan.handle, 0, None, 0, ctypes.byref(need)) == 0 and need.value > 16
    assert all(len(plan.layer_params(li)) == need.value for li in range(18))
    buf = ctypes.create_string_buffer(need.value)
    assert N.lib.msi_net_plan_layer_params(plan.handle, 0, buf, need.value - 1, None) != 0 and "needed" in N.last_error()
    assert N.lib.msi_net_plan_layer_params(plan.handle, 18, buf, need.value, None) != 0
    assert N.lib.msi_net_plan_layer_params(plan.handle, 0, None, 0, None) != 0 and N.lib.msi_net_plan_layer_params(None, 0, buf, need.value, None) != 0
    # inlaunch, fuse_ln, skip_apply, ln_blocks behind the kernel argument: the fp32 head fuses its source's LayerNorm, whose ln_apply launch is skipped
    tail = lambda li: list(np.frombuffer(plan.layer_params(li)[-16:], np.int32))
    assert tail(17)[1] == 1 and tail(16)[2] == 1 and tail(17)[3] == 0 and tail(0)[3] > 0


@pytest.mark.parametrize("which", ["A", "D"])
def test_packed_weights_are_the_recorded_bits(native_lib, which):
    """msi_net_pack_weights_host on numpy.random.default_rng(0) parameters, for descriptions A (fp32 CoordNet) and D (bf16, wrap padding) of
    tests/test_plan_decomposition.py: the SHA-256 of the whole packed blob -- tap-kernel rows, bf16 / fp16 split planes, LayerNorm windows, CoordNet
    tables -- is the one recorded in tests/golden/plan_digests.json before the packer moved to csrc/cnn_net.hip (tools/plan_golden.py)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import plan_golden
    assert plan_golden.weights_digest(which) == plan_golden.golden()["weights|" + which]


def test_plan_options_and_raw_layer_bookkeeping(native_lib):
    """Host logic of the plan object (no GPU needed: the CU count falls back to the default part): option validation, and
    which producers are left un-normalised in memory -- exactly those whose EVERY consumer applies the LayerNorm while
    staging a halo patch (or is the fused head) -- per MSI_NET_OPT_HALO."""
    import ctypes
    from matryodshka_amd import nets, _native as N
    lib = native_lib.lib
    names = nets.LAYER_NAMES

    def raw_layers(desc, halo, split3=0):
        """(split3 = 0: the native fp32 arithmetic, whose conv-transposes and small stride-2 grids stay on the tap kernel)"""
        h = ctypes.c_void_p()
        assert lib.msi_net_plan_create(desc, ctypes.byref(h)) == 0
        try:
            assert lib.msi_net_plan_set_option(h, N.NET_OPT_F32_SPLIT3, split3) == 0
            assert lib.msi_net_plan_set_option(h, N.NET_OPT_HALO, halo) == 0
            return [names[i] for i in range(17) if lib.msi_net_plan_layer_is_normalized(h, i) == 0]
        finally:
            lib.msi_net_plan_destroy(h)

    desc = nets.make_desc(1, 320, 640, 192, 64, 64, True)                 # BASELINE configs[1]
    assert raw_layers(desc, 0) == ["conv8_2"]                             # only the fused head applies on load
    # halo conv layers: producers whose only consumer is a stride-1 3x3 layer (the encoder skips feed a conv-transpose too)
    assert raw_layers(desc, 1) == ["conv3_1", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1", "conv8_2"]
    # + conv-transpose halo layers (bit 1, opt-in: measured slower than tap kernel + ln_apply): their decoder inputs and the
    # skip tensors as well -- what is left normalised in memory are the three producers whose consumer is a stride-2 layer
    # (conv1_1, conv2_1, conv3_2): three ln_apply launches per forward
    assert raw_layers(desc, 3) == ["conv1_2", "conv2_2", "conv3_1", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv6_1",
                                   "conv6_2", "conv6_3", "conv7_1", "conv7_2", "conv8_1", "conv8_2"]
    # HALO_SKIP takes layers out again: conv6_2 (layer 11) back on the tap kernel needs conv6_1 normalised in memory
    h = ctypes.c_void_p()
    assert lib.msi_net_plan_create(desc, ctypes.byref(h)) == 0
    # bit 2 (r03): the stride-2 layers on conv_halo_s2_kernel where the grid needs no K split -- conv1_2 and conv2_2 at this size
    # (conv3_3: 400 tiles, tap kernel) -- so conv1_1 and conv2_1 stay raw as well; 5 is the default
    assert raw_layers(desc, 5) == ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1", "conv8_2"]
    # the DEFAULT plan (r04): every 3x3 layer and every SAME conv-transpose stages its patch through registers for the six-product
    # bf16 split (conv_halo_x3_kernel, conv_halo_s2_x3_kernel, convt_halo_x3_kernel): no producer is normalised in memory -- no
    # ln_apply launch at all at configs[1]
    assert [names[i] for i in range(17) if lib.msi_net_plan_layer_is_normalized(h, i) == 0] == names[:17] == raw_layers(desc, 5, 0x3ffff)
    assert lib.msi_net_plan_set_option(h, N.NET_OPT_F32_SPLIT3, 0) == 0
    assert [names[i] for i in range(17) if lib.msi_net_plan_layer_is_normalized(h, i) == 0] == raw_layers(desc, 5)
    assert lib.msi_net_plan_set_option(h, N.NET_OPT_HALO_SKIP, 1 << 11) == 0
    assert [names[i] for i in range(17) if lib.msi_net_plan_layer_is_normalized(h, i) == 0] == \
        ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv4_2", "conv6_2", "conv7_1", "conv8_1", "conv8_2"]
    lib.msi_net_plan_destroy(h)
    big = nets.make_desc(1, 1024, 2048, 48, 16, 64, True)                 # a larger frame: every stride-2 layer has a large grid
    assert raw_layers(big, 5) == ["conv1_1", "conv2_1", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1", "conv8_2"]
    # msi_train_net (wrap padding): its conv-transposes normalise over the uncropped output and stay on the tap kernel
    wrap = nets.make_desc(1, 320, 640, 192, 64, 64, False)
    assert raw_layers(wrap, 3) == ["conv3_1", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1", "conv8_2"]
    small = nets.make_desc(1, 16, 24, 24, 8, 12, True)                    # nothing tiles into 4 x 16 patches
    assert raw_layers(small, 3) == ["conv8_2"]
    # configs[2] (r03: raw outputs are fp16, so the 256x64 tile stages them too: conv8_2's source conv8_1 stays raw; the
    # conv-transposes read bf16 copies -- the 128x64 one can stage raw sources as well, option BF16_STAGE_RAW bit 1, measured slower)
    bf = nets.make_desc(16, 320, 640, 384, 128, 64, True, dtype="bf16")
    assert raw_layers(bf, 1) == ["conv3_1", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1"] == raw_layers(bf, 3)
    # + the stride-2 layers on conv_halo_bf16_s2_kernel (bit 2, default): their producers conv1_1, conv2_1, conv3_2
    assert raw_layers(bf, 5) == ["conv1_1", "conv2_1", "conv3_1", "conv3_2", "conv4_1", "conv4_2", "conv6_1", "conv6_2", "conv7_1", "conv8_1"]
    # the retired keys of measured-slower experiments: asking for one is an error, not a silent no-op
    h = ctypes.c_void_p()
    assert lib.msi_net_plan_create(desc, ctypes.byref(h)) == 0
    for opt in (N.NET_OPT_APPLY_AHEAD, N.NET_OPT_F32_TILE):
        rc = lib.msi_net_plan_set_option(h, opt, 1)
        assert rc == -3 and b"experiment" in lib.msi_last_error_string()
    lib.msi_net_plan_destroy(h)
    h = ctypes.c_void_p()
    assert lib.msi_net_plan_create(desc, ctypes.byref(h)) == 0
    for opt, bad in ((N.NET_OPT_HALO, 8), (N.NET_OPT_BIGTILE, 3), (N.NET_OPT_NUM_CUS, 2), (N.NET_OPT_BF16_WAVES, 6), (99, 0)):
        assert lib.msi_net_plan_set_option(h, opt, bad) == -1
    assert lib.msi_net_plan_layer_is_normalized(h, 17) == -1 and lib.msi_net_plan_layer_is_normalized(None, 0) == -1
    lib.msi_net_plan_destroy(h)


# ---- the ONE order of the argument checks of the *_render_views entry points (include/msi_hip.h lists each one's instance): two faults at once,
# the earlier one is reported.  No launch: every call fails its validation (the dummy pointers are never dereferenced).
def _view_call(lib, name, out=True, fmt=1, views=2, size=16, planes=4, out_h=16, out_w=32, big=False):
    """`size`: the layer height (cube: the face size); big: a 4096 x 4096 layer (cube: six 4096 x 4096 fp32 faces, beyond 2^31 bytes)."""
    p = [4096 * (k + 1) for k in range(12)]
    o = (p[10], p[11]) if out else (None, None)
    h, w = (4096, 4096) if big else (size, 32)
    if name == "msi_render_views_f32":
        return lib.msi_render_views_f32(p[0], p[1], p[2], p[3], p[4], p[5], 2, views, h, w, planes, 0, out_h, out_w, o[0], o[1], None, None)
    if name == "msi_render_views_packed":
        return lib.msi_render_views_packed(p[0], fmt, p[1], p[2], p[3], p[4], p[5], 2, views, h, w, planes, 0, out_h, out_w, o[0], o[1], None, None)
    if name == "msi_render_ods_views":
        return lib.msi_render_ods_views(p[0], fmt, p[1], p[2], p[3], p[4], p[5], 2, views, h, w, planes, out_h, out_w, o[0], o[1], None, None)
    if name == "msi_render_views_sparse":
        return lib.msi_render_views_sparse(p[0], p[1], p[2], fmt, p[3], p[4], p[5], None, p[6], p[7], 2, views, h, w, planes, 0, out_h, out_w,
                                           o[0], o[1], None, None)
    if name == "msi_cube_render_views":
        return lib.msi_cube_render_views(p[0], 0 if big else fmt, p[1], p[2], p[3], p[4], p[5], p[6], 2, views, h, planes, 0, out_h, out_w,
                                         o[0], o[1], None, None)
    return lib.msi_mpi_render_views(p[0], fmt, p[1], p[2], p[3], p[4], 2, views, h, w, planes, out_h, out_w, o[0], o[1], None)


@pytest.mark.parametrize("name", ["msi_render_views_f32", "msi_render_views_packed", "msi_render_ods_views", "msi_render_views_sparse",
                                  "msi_cube_render_views", "msi_mpi_render_views"])
def test_view_entry_points_check_their_arguments_in_one_order(native_lib, name):
    def reports(text, code=-1, **kw):
        assert _view_call(native_lib.lib, name, **kw) == code, (name, kw)
        msg = native_lib.last_error()
        assert name[len("msi_"):].replace("_f32", "") + ":" in msg and text in msg, (name, kw, msg)

    has_format = name != "msi_render_views_f32"                      # (it takes fp32 stacks only: no format to be unknown)
    reports("both outputs are NULL", out=False, fmt=7, size=0 if not has_format else 16)
    if has_format:
        reports("unknown format 7", fmt=7, size=0)
    reports("bad dims", size=0, views=0)
    reports("views must be >= 1", views=0, out_h=0)
    reports("bad output size", out_h=0, big=True)
    reports("2^31 bytes" if name == "msi_cube_render_views" else "2^24", big=True)   # (control: the layer alone IS refused)
    if name in ("msi_cube_render_views", "msi_mpi_render_views"):
        reports("at most 128 planes", code=-3, planes=129, views=0)
