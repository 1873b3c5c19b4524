"""CPU checks of the C-ABI boundary, each once for the whole header: the library builds for gfx950, loads and exports every
symbol include/nudf.h declares; one version in header, package and library; every argument struct's ctypes mirror against a
C compile of the header and against the table the library reports; the loader's refusals; the hand-copied constants; and the
product path refuses to run without a GPU (no fallback)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADER = open(os.path.join(ROOT, "include", "nudf.h")).read()


def header_structs():
    """{NudfX: [field, ...]} of every `typedef struct NudfX {...} NudfX;` of the header, in its order.  A declaration may
    hold several declarators (`int32_t M, N, K;`) and arrays (`origin[3]`, `prob[NUDF_TN_MAX_PROBLEMS]`)."""
    out = {}
    for cname, body in re.findall(r"typedef struct (Nudf\w+) \{(.*?)\} \1;", HEADER, re.S):
        body = re.sub(r"\[[^\]]*\]", "", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        out[cname] = [re.findall(r"[A-Za-z_]\w*", part)[-1] for decl in body.split(";") if decl.strip()
                      for part in decl.split(",")]
    return out


def header_constants():
    """({NUDF_X: n} of every `NUDF_X = n` enum entry and every `#define NUDF_X n` of the header, the enum entries' names)"""
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    enums = {k: int(v) for k, v in re.findall(r"\b(NUDF_\w+) = (\d+)", code)}
    defines = {k: int(v) for k, v in re.findall(r"^#define (NUDF_\w+) (\d+)\b", code, re.M)}
    assert enums and defines and not set(enums) & set(defines)
    return {**enums, **defines}, set(enums)


def mirror_of(cname):
    from neuraludf_amd import _lib
    return getattr(_lib, cname[len("Nudf"):])               # the mirror of NudfX is _lib.X, without exception


def mirror_fields(st):
    return ["in" if f[0] == "in_" else f[0] for f in st._fields_]       # `in` is a Python keyword: the mirrors say in_


def test_library_builds_and_exports_header_symbols():
    from neuraludf_amd import build, _lib
    path = build.build()
    assert os.path.exists(path)
    lib = _lib.lib()
    declared = sorted(set(re.findall(r"\b(nudf_[a-z0-9_]+)\s*\(", HEADER)))
    assert declared, "no declarations found"
    for s in declared:
        assert hasattr(lib, s), f"{s} declared in include/nudf.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared
    assert sorted(_lib.SYMBOLS) == declared


def test_one_version_in_header_package_and_library():
    from neuraludf_amd import build, _lib
    build.build()
    version = header_constants()[0]["NUDF_ABI_VERSION"]
    assert version == _lib.ABI_VERSION == _lib.lib().nudf_version()


def test_struct_list_is_the_same_everywhere():
    """the typedefs of the header, its NUDF_ABI_STRUCTS list and the ctypes.Structure subclasses of _lib: a struct forgotten
    in any of the three fails here"""
    import ctypes as C
    from neuraludf_amd import _lib
    listed = re.search(r"#define NUDF_ABI_STRUCTS\(X\)((?:.*\\\n)*.*)", HEADER).group(1)
    listed = re.findall(r"X\((\w+)\)", listed)
    assert listed == list(header_structs()) and len(listed) == len(set(listed)) == 31
    classes = {"Nudf" + k for k, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert classes == set(listed) == set(_lib.MIRRORS)
    assert all(_lib.MIRRORS[c] is mirror_of(c) for c in listed)


def test_library_struct_table_equals_the_mirrors():
    """what nudf_abi_struct reports, as the loader reads it, against ctypes.sizeof of every mirror -- the step capacity of
    NudfChain included, which sets its size"""
    import ctypes as C
    from neuraludf_amd import build, _lib
    build.build()
    lib = _lib.lib()
    version, table = _lib._abi_report(lib)
    assert version == _lib.ABI_VERSION
    assert table == {c: C.sizeof(mirror_of(c)) for c in header_structs()} and len(table) == 31
    assert list(table) == list(header_structs())
    assert C.sizeof(_lib.Chain) == C.sizeof(_lib.ChainStep) * _lib.CH_MAX_STEPS + _lib.Chain.step.offset
    name = C.c_char_p()
    assert lib.nudf_abi_struct(31, C.byref(name)) == -1 and lib.nudf_abi_struct(-1, C.byref(name)) == -1
    assert lib.nudf_abi_struct(0, None) == C.sizeof(_lib.GemmNN)


def test_loader_refusals():
    """_abi_mismatch is pure: made-up reports give a refusal that names the offending item, the real values pass"""
    import ctypes as C
    from neuraludf_amd import _lib
    v = _lib.ABI_VERSION
    good = {c: C.sizeof(m) for c, m in _lib.MIRRORS.items()}
    assert _lib._abi_mismatch(v, good) is None
    for other in (v - 1, v + 1, 0):
        why = _lib._abi_mismatch(other, good)
        assert f"version {other}" in why and str(v) in why
    assert f"version {v - 1}" in _lib._abi_mismatch(v - 1, {})          # an older library has no table: refused by version
    why = _lib._abi_mismatch(v, {**good, "NudfComposite": good["NudfComposite"] + 8})
    assert "NudfComposite" in why and str(good["NudfComposite"] + 8) in why and str(good["NudfComposite"]) in why
    why = _lib._abi_mismatch(v, {**good, "NudfNewThing": 64})
    assert "NudfNewThing" in why
    why = _lib._abi_mismatch(v, {c: s for c, s in good.items() if c != "NudfPointCloud"})
    assert "NudfPointCloud" in why
    assert "NudfGemmNN" in _lib._abi_mismatch(v, {})


def test_python_constants_equal_the_header():
    """every hand-copied constant of _lib against the enum entries and #defines of include/nudf.h"""
    import ctypes as C
    from neuraludf_amd import _lib
    hdr, enums = header_constants()

    def family(prefix, skip=()):
        return {k[len(prefix):]: hdr[k] for k in enums if k.startswith(prefix) and not k[len(prefix):].startswith(skip)}

    assert _lib.EPI == family("NUDF_EPI_")
    assert _lib.CH == family("NUDF_CH_", skip="INIT_") and "SEED" in _lib.CH
    assert _lib.CH_INIT == family("NUDF_CH_INIT_")
    assert {k.upper(): v for k, v in _lib.LW.items()} == family("NUDF_LW_", skip="COUNT")
    assert max(_lib.LW.values()) < _lib.LW_COUNT == hdr["NUDF_LW_COUNT"]
    status = family("NUDF_STATUS_")
    assert status == {k[len("STATUS_"):]: v for k, v in vars(_lib).items() if k.startswith("STATUS_")} and len(status) == 3
    for name in ("CH_MAX_STEPS", "CH_STATE16", "CH_P4_X1", "CH_P4_C1", "TN_MAX_PROBLEMS", "ADAM_MAX_TENSORS",
                 "ADAM_MAX_GROUPS", "PACK_MAX_LAYERS", "PACK_MAX_FRAGS"):
        assert getattr(_lib, name) == hdr["NUDF_" + name], name
    assert _lib.CH_MAX_STEPS >= 19               # forward + input gradient of a 9-layer UDF network in one launch
    assert C.sizeof(_lib.Chain) <= 4096          # travels by value in the kernel-argument segment


def test_ctypes_structs_match_header_field_counts():
    structs = header_structs()
    assert len(structs) == 31
    for cname, names in structs.items():
        assert names == mirror_fields(mirror_of(cname)), cname


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{(NudfX, field): (offset, size), (NudfX, "sizeof"): (0, sizeof)} of every struct as gcc lays out include/nudf.h:
    one compile for the module"""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc on this box")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nudf.h"', 'int main(void) {']
    for cname, names in header_structs().items():
        lines.append('  printf("%s sizeof 0 %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, n, cname, n, cname, n)
                  for n in names]
    lines += ['  return 0;', '}']
    tmp = tmp_path_factory.mktemp("layout")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        a, b, off, size = ln.split()
        got[(a, b)] = (int(off), int(size))
    return got


@pytest.mark.parametrize("cname", list(header_structs()))
def test_struct_layout_matches_the_header(c_layout, cname):
    """sizeof, and the offset and the size of every field, of one argument struct as gcc lays out include/nudf.h, against
    its ctypes mirror in neuraludf_amd/_lib.py (the field-name test above cannot see padding or type widths; the sizes
    catch a mirror typed int32 where the header says int64_t and padding hides it from the offsets)."""
    import ctypes as C
    st, names = mirror_of(cname), header_structs()[cname]
    assert c_layout[(cname, "sizeof")] == (0, C.sizeof(st))
    assert names == mirror_fields(st)
    for n, f in zip(names, st._fields_):
        field = getattr(st, f[0])
        assert c_layout[(cname, n)] == (field.offset, field.size), n


def test_weight_gradient_gemm_plan_host_logic():
    """the planner of nudf_gemm_tn_grouped is host code: workspace sizes (= workgroups x slot) of known groups, one
    resident wave of <= 512 workgroups, argument errors -- no GPU involved."""
    import ctypes as C
    from neuraludf_amd import _lib
    lib = _lib.lib()
    SLOT = 128 * 128 + 128

    def group(shapes, M, flags=0, ld=None):
        g = _lib.GemmTNGroup()
        g.n_problems, g.M, g.rows_per_block, g.prec = len(shapes), M, 0, 0
        for i, (NA, NB) in enumerate(shapes):
            q = g.prob[i]
            q.A1, q.B1, q.C = 4096, 8192, 16384          # fake 16-byte aligned addresses: never dereferenced here
            q.lda1, q.ldb1, q.ldc = ld or (NA + 3) // 4 * 4, ld or (NB + 3) // 4 * 4, NB
            q.NA, q.NB, q.flags = NA, NB, flags
        return g

    udf = [(256, 40)] + [(256, 256)] * 3 + [(217, 256)] + [(256, 256)] * 3 + [(256, 256), (1, 256)]
    n = lib.nudf_gemm_tn_grouped_workspace(C.byref(group(udf, 65536)))
    assert n % SLOT == 0 and 36 * 8 <= n // SLOT <= 512          # 36 tiles, several row chunks each, one resident wave
    small = lib.nudf_gemm_tn_grouped_workspace(C.byref(group([(3, 5)], 17)))
    assert small == SLOT                                         # one tile, one chunk (at least 8 k-steps per workgroup)
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(group([], 100))) == 0
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(group([(1024, 1024)] * 2, 100))) < 0     # 128 tiles > 64
    assert b"64 output tiles" in lib.nudf_last_error()
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(group([(64, 64)], 100, ld=66))) < 0       # ld % 4
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(group([(64, 64)], 100, flags=1 | 4))) < 0  # blocked is fp32-only
    # 16-bit launches and bf16 operands use whole quadrants and equal costs: still one resident wave
    g16 = group(udf, 262144, flags=3, ld=256)
    g16.prec = 2
    assert 0 < lib.nudf_gemm_tn_grouped_workspace(C.byref(g16)) // SLOT <= 512
    # with a workspace (fixed-order, non-atomic reduction) the problems of a group must write disjoint C / dbias ranges
    g2 = group([(64, 64), (64, 64)], 4096)
    g2.workspace = 1 << 20                                # fake non-NULL pointer: the planner never dereferences it
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g2)) < 0           # both problems write C = 16384
    assert b"disjoint" in lib.nudf_last_error()
    g2.prob[1].C = 16384 + 4 * 64 * 64
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g2)) > 0
    g2.prob[0].dbias, g2.prob[1].dbias = 1 << 16, (1 << 16) + 4 * 32       # [NA = 64] ranges overlap by 32 entries
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g2)) < 0
    g2.prob[1].dbias = (1 << 16) + 4 * 64
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g2)) > 0
    g2.workspace = None                                   # atomics path: overlapping outputs are allowed
    g2.prob[1].C = 16384
    assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g2)) > 0


def test_retired_tn_flag_bits_are_masked_off():
    """bits 2 (drop the epilogue) and 4 (skip the bias sums) of nudf_set_tn_flags computed wrong results on purpose, bit 1024
    selected the wide bf16x3 kernel that was deleted; all three are retired: the setter drops them, so an old command line
    can neither produce garbage nor ask for a kernel that is gone.  Host-only call."""
    from neuraludf_amd import _lib
    lib = _lib.lib()
    prev = lib.nudf_set_tn_flags(2 | 4 | 16 | 1024)
    try:
        assert lib.nudf_set_tn_flags(0) == 16
    finally:
        lib.nudf_set_tn_flags(prev)


def test_per_layer_weight_gradient_gemm_refuses_formatted_operands():
    """nudf_gemm_tn reads row-major fp32 only: the per-layer fallback must refuse bf16-stored / blocked-layout state
    instead of producing silent garbage."""
    from neuraludf_amd import mlp
    from neuraludf_amd._lib import NudfError
    a = torch.zeros(64, 32)
    with pytest.raises(NudfError, match="gemm_tn_grouped"):
        mlp.gemm_tn(a.to(torch.bfloat16), 32, a, torch.zeros(32, 32), 32, 32, 64)
    with pytest.raises(NudfError, match="gemm_tn_grouped"):
        mlp.gemm_tn(a, 32, mlp.block(a), torch.zeros(32, 32), 32, 32, 64)


def test_weight_gradient_gemm_workgroup_order_host_logic():
    """blockIdx -> (tile, row chunk) of nudf_gemm_tn_grouped (host mirror of the kernels' decode): the live workgroups are a
    bijection onto the workspace slots, the tiles of a problem that read the same row chunk share blockIdx % 8 = the XCD --
    EVERY chunk (round 5: the last, narrower column of eight keeps its lanes and leaves holes, which exit) -- and no XCD
    receives more live workgroups than it has slots (2 per CU x 32 CUs)."""
    import collections
    import ctypes as C
    from neuraludf_amd import _lib
    lib = _lib.lib()

    def plan(shapes, M, flags=0, prec=0, ld=None):
        g = _lib.GemmTNGroup()
        g.n_problems, g.M, g.rows_per_block, g.prec = len(shapes), M, 0, prec
        for i, (NA, NB) in enumerate(shapes):
            q = g.prob[i]
            q.A1, q.B1, q.C = 4096, 8192, 16384
            q.lda1, q.ldb1, q.ldc = ld or (NA + 3) // 4 * 4, ld or (NB + 3) // 4 * 4, NB
            q.NA, q.NB, q.flags = NA, NB, flags
        out = (C.c_int32 * (4 * 2048))()
        n = lib.nudf_gemm_tn_grouped_plan(C.byref(g), out, 2048)
        assert 0 < n <= 2048
        assert lib.nudf_gemm_tn_grouped_workspace(C.byref(g)) % sum(1 for b in range(n) if out[4 * b] >= 0) == 0
        return [tuple(out[4 * b:4 * b + 4]) for b in range(n)]

    udf = [(256, 40)] + [(256, 256)] * 3 + [(217, 256)] + [(256, 256)] * 3 + [(256, 256), (1, 256)]
    color = [(256, 295)] + [(256, 256)] * 3 + [(3, 256)]
    for shapes, M, kw in [(udf, 65536, {}), (udf, 65536, dict(prec=3)), (color, 65536, dict(prec=3)), (udf, 5000, {}),
                          ([(129, 72), (3, 128), (256, 256)], 777, {}), (udf, 262144, dict(flags=3, prec=2, ld=256)),
                          ([(256, 256)], 65536, dict(prec=3)), ([(512, 384)] * 2, 40000, dict(prec=3))]:
        grid = plan(shapes, M, **kw)
        live = [(bid, b) for bid, b in enumerate(grid) if b[0] >= 0]
        assert all(b == (-1, -1, -1, -1) for b in grid if b[0] < 0)
        assert len(live) <= 512 and len(grid) <= len(live) * 1.5 + 64
        assert sorted(b[3] for _, b in live) == list(range(len(live)))                      # every slot exactly once
        per_chunk = collections.defaultdict(set)
        chunks_of = collections.Counter((b[0], b[1]) for _, b in live)
        for bid, (prob, tile, chunk, _) in live:
            per_chunk[(prob, chunks_of[(prob, tile)], chunk)].add((tile, bid % 8))
        shared = 0
        for (prob, n_chunks, chunk), members in per_chunk.items():
            if len(members) > 1:
                assert len({x for _, x in members}) == 1, (prob, chunk, members)
                shared += 1
        if M >= 5000 and len(shapes) > 1:
            assert shared > 0
        per_xcd = collections.Counter(bid % 8 for bid, _ in live)
        assert max(per_xcd.values()) <= 64, per_xcd
        if len(live) > 256:
            assert min(per_xcd.values()) >= 0.75 * max(per_xcd.values()), per_xcd


def test_blocked_layout_helpers_are_inverse():
    from neuraludf_amd import mlp
    t = torch.arange(128 * 24, dtype=torch.float32).reshape(128, 24)
    b = mlp.block(t)
    assert mlp._isblk(b) and not mlp._isblk(t) and b.shape == t.shape
    r, c = 77, 13                                                   # the formula of include/nudf.h
    assert float(b.reshape(-1)[(r // 32) * 32 * 24 + (c // 4) * 128 + (r % 32) * 4 + c % 4]) == float(t[r, c])
    assert torch.equal(mlp.unblock(b), t)
    assert mlp.unblock(t) is t


def test_no_cpu_fallback():
    from neuraludf_amd._lib import NudfError
    from neuraludf_amd.train import Trainer
    from neuraludf_amd import synth
    tr = Trainer(torch.device("cpu"), dict(n_samples=16, n_importance=0, n_outside=0, up_sample_steps=1, perturb=0.0))
    rays = synth.make_rays(synth.make_scene("tiny"), 0, 4)
    with pytest.raises(NudfError):
        tr.loss(rays)


def test_product_never_imports_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "neuraludf_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle", src, re.M):
                    bad.append(f)
    assert not bad, bad
