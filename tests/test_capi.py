"""CPU suite: the C-ABI library loads here (no GPU), exports every symbol the header declares and is typed from it;
the product never reaches into oracle/."""
import ast
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared():
    from jtsm_amd import _lib

    return sorted(_lib.declarations())


def test_library_loads_and_exports_all_declared_symbols():
    from jtsm_amd import _lib

    lib = _lib.lib()
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing
    assert len(_declared()) >= 15
    assert b"gfx950" in lib.jtsm_version()


def test_code_object_targets_gfx950_only():
    from jtsm_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # offload-bundle entries name their target; rocPRIM's host-side dispatch tables carry other architectures' NAMES
    # as plain strings, which is not code for them
    for other in (b"gfx942", b"gfx90a", b"gfx1100"):
        assert b"amdgcn-amd-amdhsa--" + other not in blob
    assert b"sm_80" not in blob and b"nvptx" not in blob


def test_cpu_tensors_are_refused_not_silently_computed():
    import torch

    from jtsm_amd.layers import MOIPool, ROIAlign, ROIAlignRotated

    with pytest.raises(RuntimeError):
        ROIAlign((7, 7), 1.0, 0)(torch.zeros(1, 1, 5, 5), torch.zeros(1, 5))
    with pytest.raises(RuntimeError):
        ROIAlignRotated((7, 7), 1.0, 0)(torch.zeros(1, 1, 5, 5), torch.zeros(1, 6))
    with pytest.raises(RuntimeError):
        MOIPool((7, 7), 1.0)(torch.zeros(1, 1, 5, 5), torch.zeros(1, 5),
                             torch.zeros(1, 4, dtype=torch.int32),
                             torch.zeros(1, 20, 20, dtype=torch.int32))


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "jtsm_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "liboracle" in txt \
                        or re.search(r'#include\s+".*oracle', txt):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_conv_planning_host_logic_handles_empty_and_odd_shapes():
    """jtsm_conv_workspace_bytes / jtsm_conv_plan are pure host code: an empty batch (a rank with no
    foreground roi) must plan to 'nothing', not divide by zero; a real layer plans a sane tile / split."""
    from jtsm_amd import _lib
    from jtsm_amd.layers.conv import ConvShape

    lib = _lib.lib()
    for kh, stride, pad in ((1, 1, 0), (3, 1, 1), (1, 2, 0), (2, 2, 0)):
        s = ConvShape(0, 14, 14, 256, 256, kh, kh, stride, pad, 1)
        for bwd in (0, 1):
            assert lib.jtsm_conv_workspace_bytes(C.byref(s), bwd) == 0
        for role in (0, 1, 2):
            k, tm, tn, sp = C.c_int(-1), C.c_int(), C.c_int(), C.c_int()
            assert lib.jtsm_conv_plan(C.byref(s), role, 0, C.byref(k), C.byref(tm), C.byref(tn), C.byref(sp)) == 0
            assert sp.value == 1
    # res5 3x3 at 2x(32x32): few output tiles -> split-K with a workspace of splits * M * N floats
    s = ConvShape(2, 32, 32, 512, 512, 3, 3, 1, 1, 1)
    k, tm, tn, sp = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.jtsm_conv_plan(C.byref(s), 0, 0, C.byref(k), C.byref(tm), C.byref(tn), C.byref(sp)) == 0
    assert (tm.value, tn.value) == (128, 128) and 1 < sp.value <= 16
    assert lib.jtsm_conv_workspace_bytes(C.byref(s), 0) == sp.value * 2048 * 512 * 4
    bad = ConvShape(1, 8, 8, 3, 8, 1, 1, 1, 0, 1)  # in_c not a multiple of 4
    assert lib.jtsm_conv_plan(C.byref(bad), 0, 0, None, None, None, None) != 0
    assert b"in_c" in lib.jtsm_last_error()


def test_bf16x3_plan_reports_the_ring_for_long_k_64_tiles():
    """jtsm_conv_bf16x3_plan (host code): the res4 / res5 1x1 layers that run on 64 x 64 tiles take the four-stage
    ring (NBUF = 4) from four stages per K slice; the GPU conv cases `ring_*` in tests/test_hip_conv.py are such
    shapes; large layers stay double-buffered on 256 x 256 tiles."""
    from jtsm_amd import _lib
    from jtsm_amd.layers.conv import ConvShape

    lib = _lib.lib()

    def plan(shape, role):
        v = [C.c_int() for _ in range(6)]
        assert lib.jtsm_conv_bf16x3_plan(C.byref(ConvShape(*shape)), role, *[C.byref(x) for x in v]) == 0
        return tuple(x.value for x in v)   # wm, wn, tm, tn, nbuf, splits

    # BASELINE layers: res4 conv1 (1024 -> 256 on 2 x 64 x 64), res5 conv1 (2048 -> 512 on 2 x 32 x 32), forward
    assert plan((2, 64, 64, 1024, 256, 1, 1, 1, 0, 1), 0) == (2, 2, 1, 1, 4, 1)
    assert plan((2, 32, 32, 2048, 512, 1, 1, 1, 0, 1), 0) == (2, 2, 1, 1, 4, 2)
    # data gradient of res4 conv3 (256 -> 1024): contracted over the 1024 output channels
    assert plan((2, 64, 64, 256, 1024, 1, 1, 1, 0, 1), 1) == (2, 2, 1, 1, 4, 1)
    # the GPU suite's ring cases
    assert plan((2, 16, 16, 1024, 256, 1, 1, 1, 0, 1), 0) == (2, 2, 1, 1, 4, 8)
    assert plan((1, 20, 20, 352, 128, 1, 1, 1, 0, 1), 0) == (2, 2, 1, 1, 4, 2)
    assert plan((1, 12, 12, 64, 128, 3, 3, 1, 1, 1), 0) == (2, 2, 1, 1, 4, 4)
    # FPN p2 output conv: the halo kernel (reported as NBUF = 0); a res2-sized 1x1 (8 stages, 2048 tiles): 128 x 128
    # tiles, double-buffered
    assert plan((2, 256, 256, 256, 256, 3, 3, 1, 1, 1), 0)[4] == 0
    assert plan((2, 256, 256, 256, 256, 1, 1, 1, 0, 1), 0)[:5] == (2, 2, 2, 2, 2)


# Group sizes the weight-gradient group queries are recorded at (8 = kMaxGroup, csrc/conv_x3.h).
PLAN_GROUP_SIZES = (1, 2, 3, 6, 8)
CONV_PLAN_TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.npz")


def conv_plan_answers(lib, shape):
    """Everything the host-side planning and workspace queries say about one jtsm_conv_shape, as a flat list of
    integers (output arguments a failing call leaves alone read -1): jtsm_conv_plan for roles 0-2 x has_kscale 0/1,
    jtsm_conv_bf16x3_plan for roles 0-2, the weight-gradient group plan and workspace for PLAN_GROUP_SIZES, the four
    single-layer workspace sizes, jtsm_conv_bf16x3_colsum_rows and jtsm_conv_bf16x3_eligible."""
    from jtsm_amd.layers.conv import ConvShape

    ref = C.byref(ConvShape(*[int(v) for v in shape]))
    row = []

    def outs(n):
        o = [C.c_int(-1) for _ in range(n)]
        return o, [C.byref(x) for x in o]

    for role in (0, 1, 2):
        for has_kscale in (0, 1):
            o, (k, tm, tn, sp) = outs(4)
            row.append(lib.jtsm_conv_plan(ref, role, has_kscale, k, tm, tn, sp))
            row.extend(x.value for x in o)
    for role in (0, 1, 2):
        o, (wm, wn, tm, tn, nbuf, sp) = outs(6)
        row.append(lib.jtsm_conv_bf16x3_plan(ref, role, wm, wn, tm, tn, nbuf, sp))
        row.extend(x.value for x in o)
    for n in PLAN_GROUP_SIZES:
        o, (tile, sp) = outs(2)
        row.append(lib.jtsm_conv_bf16x3_wgrad_group_plan(ref, n, tile, sp))
        row.extend(x.value for x in o)
        row.append(lib.jtsm_conv_bf16x3_wgrad_group_workspace_bytes(ref, n))
    row += [lib.jtsm_conv_workspace_bytes(ref, 0), lib.jtsm_conv_workspace_bytes(ref, 1),
            lib.jtsm_conv_bf16x3_wgrad_workspace_bytes(ref), lib.jtsm_conv_bf16x3_wgrad_bias_workspace_bytes(ref)]
    row += [lib.jtsm_conv_bf16x3_colsum_rows(ref, role) for role in (0, 1)]
    row += [lib.jtsm_conv_bf16x3_eligible(ref, role) for role in (0, 1, 2)]
    return row


def test_conv_planning_answers_match_the_recorded_table():
    """tests/golden/conv_plan_table.npz (tests/golden/make_golden.py: conv_plan_table) holds, for every convolution /
    linear shape of the BASELINE configs[2] and configs[4] steps, the shapes of the convolution tests and a grid around
    the rule boundaries, what the planning queries answered when the table was recorded.  The launchers read the same
    plan functions ("One plan per contraction launch"), so any change of a tile, slice or buffer rule shows
    here, per field.  Recorded and replayed with no JTSM_* variable set."""
    import numpy as np

    from jtsm_amd import _lib

    knobs = sorted(k for k in os.environ if k.startswith(("JTSM_X3_", "JTSM_WGRAD_")))   # (what the rules read)
    assert not knobs, "the table holds the default rules; unset %s" % knobs
    lib = _lib.lib()
    table = np.load(CONV_PLAN_TABLE)
    shapes, want = table["shapes"], table["answers"]
    assert shapes.shape[0] == want.shape[0] >= 2000 and shapes.shape[1] == 10
    got = np.array([conv_plan_answers(lib, s) for s in shapes], dtype=np.int64)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d differing fields; first: shape %s column %d: got %d, recorded %d" % (
        len(bad), shapes[bad[0][0]].tolist(), bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


WORKSPACE_SIZE_TABLE = os.path.join(ROOT, "tests", "golden", "workspace_sizes.npz")

# The argument sets of the recorded workspace-size table, per `jtsm_<name>_workspace_bytes` query: the empty cases, sizes
# one below / at / above a multiple of 64 and a mid-sized case each.  Every sorted array (D, n, R * K) holds at most 1024 items.
WORKSPACE_SIZE_CASES = {
    "voc_eval": [(0, 0, 1), (1, 1, 1), (0, 5, 3), (5, 0, 3), (63, 63, 20), (64, 64, 20), (65, 65, 20), (257, 70, 20),
                 (127, 128, 129), (1000, 300, 80), (1024, 2000, 200)],                               # D, G, C
    "coco_image": [(0, 0, 1, 0, 0, 100), (1, 1, 1, 0, 0, 100), (0, 3, 2, 0, 0, 1), (63, 64, 80, 0, 0, 100),
                   (64, 63, 80, 0, 0, 100), (65, 65, 80, 0, 0, 100), (100, 30, 80, 0, 0, 128), (5, 4, 3, 17, 13, 100),
                   (64, 65, 80, 64, 64, 100), (100, 20, 80, 480, 640, 100), (10, 10, 5, 0, 0, 129),
                   (300, 130, 80, 0, 0, 100)],                                                       # n, G, K, H, W, max_det
    "coco_accumulate": [(0, 1), (1, 1), (63, 1), (64, 80), (65, 80), (127, 64), (128, 63), (129, 65), (1000, 80),
                        (1024, 91)],                                                                 # D, K
    "pq_accumulate": [(0, 0, 1), (1, 1, 1), (0, 31, 1), (31, 0, 5), (32, 32, 10), (63, 63, 133), (64, 64, 133),
                      (65, 65, 133), (20, 30, 133), (200, 2000, 133), (1023, 1024, 133)],            # G, P, C
    "batched_nms": [(0, 1, 0), (5, 0, 5), (1, 1, 0), (1, 1, 1), (63, 1, 63), (64, 1, 64), (65, 1, 65), (130, 65, 2),
                    (128, 80, 64), (1000, 80, 100), (1024, 80, 1024)],                               # n, K, max_per_class
    "fast_rcnn_inference": [(0, 1), (1, 0), (1, 1), (63, 1), (64, 1), (65, 1), (1, 80), (50, 20), (12, 80), (16, 64),
                            (15, 65)],                                                               # R, K
    "mine_top_p": [(0, 0, 0), (1, 0, 5), (1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (2, 20, 63), (2, 20, 100),
                   (8, 80, 300)],                                                                    # B, G, t_max
    "roi_merge": [(0, 0), (1, 0), (1, 1), (1, 63), (1, 64), (1, 65), (63, 100), (64, 100), (65, 100), (2, 1000),
                  (8, 4000)],                                                                        # B, R
}
WORKSPACE_SIZE_CASES["batched_nms_rotated"] = WORKSPACE_SIZE_CASES["batched_nms"]


def workspace_size_answers(lib, name):
    query = {"voc_eval": lambda D, G, K: lib.jtsm_voc_eval_workspace_bytes(D, G, K),
             "coco_image": lambda n, G, K, H, W, m: lib.jtsm_coco_image_workspace_bytes(n, G, K, H, W, m),
             "coco_accumulate": lambda D, K: lib.jtsm_coco_accumulate_workspace_bytes(D, K),
             "pq_accumulate": lambda G, P, K: lib.jtsm_pq_accumulate_workspace_bytes(G, P, K),
             "batched_nms": lambda n, K, m: lib.jtsm_batched_nms_workspace_bytes(n, K, m),
             "batched_nms_rotated": lambda n, K, m: lib.jtsm_batched_nms_rotated_workspace_bytes(n, K, m),
             "fast_rcnn_inference": lambda R, K: lib.jtsm_fast_rcnn_inference_workspace_bytes(R, K),
             "mine_top_p": lambda B, G, t: lib.jtsm_mine_top_p_workspace_bytes(B, G, t),
             "roi_merge": lambda B, R: lib.jtsm_roi_merge_workspace_bytes(B, R)}[name]
    return [query(*args) for args in WORKSPACE_SIZE_CASES[name]]


def test_workspace_sizes_match_the_recorded_table():
    """tests/golden/workspace_sizes.npz (tests/golden/make_golden.py: workspace_size_table) holds what the workspace
    queries of the device-side sorters answered for WORKSPACE_SIZE_CASES before their layouts moved onto the one arena
    of csrc/workspace.h: every buffer, its alignment and the empty-buffer rule of each entry point show here as bytes.
    Every case keeps each sorted array at 1024 items or fewer (so below the 4096 from which the radix sort's size query
    fails on a host without a device and the answer lacks the sort's scratch — csrc/sorted_segments.h:
    sort_pairs_temp_bytes): up to 1024 items rocPRIM sorts in one block and answers a fixed 256 bytes before it asks
    for the device, above that its answer is the device's tuning (4095 items: 256 bytes without a device, 48 KiB on
    gfx950) — so the table replays identically with and without a device."""
    import numpy as np

    from jtsm_amd import _lib

    lib = _lib.lib()
    assert lib.jtsm_voc_eval_workspace_bytes(0, 0, 1) == 3840
    assert lib.jtsm_voc_eval_workspace_bytes(1, 1, 1) == 3840
    assert lib.jtsm_voc_eval_workspace_bytes(257, 70, 20) == 25088
    radix_sorted = {"voc_eval": lambda D, G, C_: D, "coco_accumulate": lambda D, K: D,      # items of the radix sorts
                    "batched_nms": lambda n, K, m: n, "batched_nms_rotated": lambda n, K, m: n,
                    "fast_rcnn_inference": lambda R, K: R * K}
    table = np.load(WORKSPACE_SIZE_TABLE)
    assert sorted(k[:-5] for k in table.files if k.endswith("_args")) == sorted(WORKSPACE_SIZE_CASES)
    for name, cases in WORKSPACE_SIZE_CASES.items():
        assert table[name + "_args"].tolist() == [list(c) for c in cases], name
        if name in radix_sorted:
            assert max(radix_sorted[name](*c) for c in cases) <= 1024, name
        got, want = workspace_size_answers(lib, name), table[name + "_bytes"].tolist()
        assert got == want, "%s: %s" % (name, [(c, g, w) for c, g, w in zip(cases, got, want) if g != w])


def test_integration_doc_maps_every_declared_symbol():
    """INTEGRATION.md's symbol <-> reference-interface table names every entry point include/jtsm_hip.h declares
    (brace lists and trailing-* families expanded)."""
    import re

    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    have = set()
    for m in re.findall(r"jtsm_[a-z0-9_{},*]+", integ):
        parts = [m]
        while any("{" in p for p in parts):
            nxt = []
            for p in parts:
                mm = re.search(r"\{([^{}]*)\}", p)
                if not mm:
                    nxt.append(p)
                    continue
                nxt += [p[:mm.start()] + alt + p[mm.end():] for alt in mm.group(1).split(",")]
            parts = nxt
        have.update(parts)
    missing = [n for n in _declared()
               if n not in have and not any("*" in w and re.fullmatch(w.replace("*", ".*"), n) for w in have)]
    assert not missing, missing


def test_every_declared_function_is_typed_from_the_header():
    """lib() gives every entry point one argtype per declared parameter and the mapped return type: size_t for the
    workspace sizes, int return codes for the rest but a handful of declared exceptions."""
    from jtsm_amd import _lib

    lib = _lib.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    params = dict(re.findall(r"\b(jtsm_[a-z0-9_]+)\s*\(([^()]*)\)", txt))
    assert sorted(params) == _declared()
    special = {"jtsm_last_error": C.c_char_p, "jtsm_version": C.c_char_p, "jtsm_event_create": C.c_void_p,
               "jtsm_event_destroy": None, "jtsm_conv_set_mid_event": None, "jtsm_conv_set_splitk_fused": None}
    for name, plist in params.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == (0 if plist.strip() == "void" else plist.count(",") + 1), name
        want = special.get(name, C.c_size_t if name.endswith("_workspace_bytes") else C.c_int)
        assert fn.restype is want, (name, fn.restype)
    assert lib.jtsm_dropout_split_f32.argtypes[4:7] == [C.c_long, C.c_float, C.c_ulonglong]


def test_size_arguments_and_results_keep_64_bits():
    """jtsm_pool_f16_workspace_bytes is host arithmetic on long element counts: an untyped call would pass and
    return them as 32-bit ints."""
    from jtsm_amd import _lib

    assert _lib.lib().jtsm_pool_f16_workspace_bytes(3 << 31, 0, 0, 0) >= 12 << 31


def test_declarations_reject_unmapped_types(tmp_path):
    from jtsm_amd import _lib

    h = tmp_path / "h.h"
    h.write_text("int jtsm_ok(const float* x, unsigned long long n, void* stream);\nint jtsm_bad(bool flag);\n")
    with pytest.raises(ValueError, match="jtsm_bad"):
        _lib.declarations(str(h))
    h.write_text("/* jtsm_comment(int a); */\n#define JTSM_X(a) jtsm_macro(a)\nint jtsm_ok(const float* x, "
                 "unsigned long long n, void* stream);\nvoid jtsm_none(void);\n")
    assert _lib.declarations(str(h)) == {"jtsm_ok": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_void_p]),
                                         "jtsm_none": (None, [])}


def test_a_declared_symbol_missing_from_the_library_fails_at_load(monkeypatch):
    from jtsm_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "declarations", lambda: {"jtsm_not_exported": (C.c_int, [])})
    with pytest.raises(RuntimeError, match="jtsm_not_exported"):
        _lib.lib()


# Calls whose entry point is picked at run time, out of the scan's sight: roi_align.py builds the name from the op and
# dtype for getattr; postprocess.py picks the u8 or f32 image preprocessing.
_PICKED_AT_RUN_TIME = {"jtsm_amd/layers/roi_align.py", "jtsm_amd/layers/postprocess.py"}
# Called by tools/sweeps/sem_side_*.py; exported only by a JTSM_DIAG_UP2 build of the library, not declared.
_UNDECLARED = {"jtsm_diag_up2_read"}


def _python_sources():
    paths = [os.path.join(ROOT, "__graft_entry__.py")]
    for top in ("jtsm_amd", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(dirpath, f) for f in files if f.endswith(".py")]
    return sorted(paths)


def test_library_calls_pass_the_declared_number_of_arguments():
    """Every `<expr>.jtsm_name(...)` call without *args in the tree passes exactly the header's parameter count: a
    typed ctypes function refuses too few arguments but silently accepts too many."""
    from jtsm_amd import _lib

    decl = _lib.declarations()
    bad, undeclared, picked = [], set(), set()
    for path in _python_sources():
        rel = os.path.relpath(path, ROOT)
        tree = ast.parse(open(path).read(), path)
        seen = set()    # attributes that are called or read further (`fn.argtypes`)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
                seen.add(id(node.func))
            if isinstance(node, ast.Attribute):
                seen.add(id(node.value))
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and node.attr.startswith("jtsm_") and id(node) not in seen:
                picked.add(rel)
            if not isinstance(node, ast.Call):
                continue
            f = node.func
            if isinstance(f, ast.Name) and f.id == "getattr" and len(node.args) > 1 and any(
                    isinstance(c, ast.Constant) and str(c.value).startswith("jtsm_") for c in ast.walk(node.args[1])):
                picked.add(rel)
            if not (isinstance(f, ast.Attribute) and f.attr.startswith("jtsm_")) or \
                    any(isinstance(a, ast.Starred) for a in node.args):
                continue
            n = len(node.args) + len(node.keywords)
            if f.attr not in decl:
                undeclared.add(f.attr)
            elif n != len(decl[f.attr][1]):
                bad.append("%s:%d %s: %d arguments, declared %d" % (rel, node.lineno, f.attr, n, len(decl[f.attr][1])))
    assert not bad, bad
    assert undeclared <= _UNDECLARED, undeclared
    assert picked == _PICKED_AT_RUN_TIME, picked
