"""CPU-side checks of the product: the C-ABI library loads and exports every symbol include/smpl_amd.h
declares, the host model compiler agrees bit for bit with the oracle, errors map to codes, and the
library refuses to work without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle_binding import Oracle
from smpl_amd import capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(smplx_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 40
    L = capi.lib()
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(capi.SYMBOLS) == declared   # the Python binding knows exactly the header's entry points


@pytest.mark.parametrize("robot", [scenes.arm7_robot, scenes.dual_arm14_robot, scenes.mixed_kinds_robot])
def test_host_model_compiler_matches_oracle_bitwise(robot, small_cfg):
    import copy
    cfg = copy.copy(small_cfg)
    cfg.robot_text = robot()
    if robot is scenes.dual_arm14_robot:
        cfg.params = scenes.PlanningParams([scenes.DEG] * 14)
        cfg.mprim = scenes.mprim_text(14, range(14), range(14))
    if robot is scenes.mixed_kinds_robot:   # rotated origins, a generic axis, a prismatic and a continuous joint
        cfg.params = scenes.PlanningParams([2 * scenes.DEG, 0.01, 2 * scenes.DEG, 2 * scenes.DEG, 2 * scenes.DEG])
        cfg.mprim = scenes.mprim_text(5, range(3), range(5))
    om = Oracle(cfg).model()
    m = capi.Model(cfg.robot_text)
    pm = m.arrays()
    fi = pm["file_index"]
    assert np.array_equal(pm["origins"], om["origins"][fi])      # joint origins (rpy -> matrix)
    assert np.array_equal(pm["k"], om["k"][fi])                  # motion-sphere factors |c| + r
    assert np.array_equal(pm["xyzr"], om["xyzr"])                # sphere trees: centres and radii, node order
    first = om["tree_first"]
    ol, orr = om["left"].copy(), om["right"].copy()
    for t in range(len(first) - 1):
        sl = slice(first[t], first[t + 1])
        ol[sl] = np.where(ol[sl] >= 0, ol[sl] + first[t], -1)
        orr[sl] = np.where(orr[sl] >= 0, orr[sl] + first[t], -1)
    assert np.array_equal(ol, pm["left"]) and np.array_equal(orr, pm["right"])
    assert np.array_equal(first, pm["tree_first"])
    assert np.array_equal(om["pairs"], pm["pairs"])
    if robot is scenes.arm7_robot:
        assert (m.njoints, m.nvars, m.ntrees, m.nnodes, m.npairs, m.nslots) == (13, 7, 8, 38, 11, 1)
        leaves = int((pm["left"] < 0).sum())
        assert leaves == 23                                       # trees of 1,4,7,3,2,2,2,2 leaves
    elif robot is scenes.dual_arm14_robot:
        assert m.nvars == 14 and m.ntrees == 16 and int((pm["left"] < 0).sum()) == 46
    else:
        assert m.nvars == 5 and m.ntrees == 6 and int((pm["left"] < 0).sum()) == 10


def test_parse_errors_and_limits_map_to_codes():
    with pytest.raises(capi.SmplxError) as e:
        capi.Model("link a\njoint j bogus a b 0 0 0 0 0 0 0 0 1 0 0\n")
    assert e.value.code == -2
    with pytest.raises(capi.SmplxError) as e:
        capi.Model("link a\nlink b\njoint j fixed a c 0 0 0 0 0 0 0 0 1 0 0\n")
    assert e.value.code == -2 and "unknown link" in str(e.value)
    too_many = "link l0\n" + "".join(
        f"link l{i}\njoint j{i} fixed l{i-1} l{i} 0 0 0 0 0 0 0 0 1 0 0\n" for i in range(1, 60))
    with pytest.raises(capi.SmplxError) as e:
        capi.Model(too_many)
    assert e.value.code == -3


def test_no_cpu_fallback_without_gpu(small_cfg):
    if capi.lib().smplx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.SmplxError) as e:
        capi.Space.from_config(small_cfg)
    assert e.value.code == -4           # SMPLX_E_HIP: fails loudly, never computes on the CPU


def test_scene_generator_is_deterministic_and_exact(small_cfg):
    again = scenes.config_small()
    assert np.array_equal(again.grid.d2, small_cfg.grid.d2)
    # exact EDT with border cells as obstacles, capped (distance_map.hpp:560-606 border, :126-127 cap)
    g = small_cfg.grid
    dmax = g.dmax_int
    rng = np.random.default_rng(5)
    occ = g.d2 == 0
    pts = np.argwhere(occ)
    for _ in range(40):
        c = rng.integers(0, g.dims[0], 3)
        best = min(int(((pts - c) ** 2).sum(1).min()) if len(pts) else 10 ** 9,
                   min(int(c[a] + 1) ** 2 for a in range(3)), min(int(g.dims[a] - c[a]) ** 2 for a in range(3)))
        assert g.d2[tuple(c)] == min(best, dmax * dmax)


def test_mprim_text_round_trip_against_oracle(small_cfg):
    o = Oracle(small_cfg)
    assert o.M == 25            # 3 adaptive slots + (4 long + 7 short) x 2 (converse), pr2.mprim layout
    assert o.N == 7


# --- per-robot kernel build (csrc/specialize.cpp): host-side pieces, no GPU ---

def _const_header(robot_text):
    import ctypes as C
    from smpl_amd import capi
    L = capi.lib()
    m = capi.Model(robot_text)
    L.smplx_model_const_header.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    n = L.smplx_model_const_header(m.h, None, 0)
    buf = C.create_string_buffer(n)
    assert L.smplx_model_const_header(m.h, buf, n) == n
    return buf.value.decode()


def test_model_constants_header_describes_the_chain(small_cfg):
    h = _const_header(small_cfg.robot_text)
    assert "#define CM_NJ 13" in h and "#define CM_NV 7" in h and "#define CM_NT 8" in h
    # 7 revolute joints with identity-rotation origins (kinds 7..9), fixed ones 6: every transform has a literal form
    assert "#define CM_NEEDS_JOINTS 0" in h
    kinds = [int(x) for x in h.split("CM_KIND[13] = {")[1].split("}")[0].strip(",").split(",")]
    assert sorted(set(kinds)) == [6, 7, 8, 9] and sum(k != 6 for k in kinds) == 7
    # doubles are hex floats: the compiled constants are the host model's bits
    assert "0x1." in h.split("CM_VAR_K")[1].split("\n")[0]


def test_shard_range_in_the_abi_matches_the_python_sharding():
    import ctypes as C
    L = capi.lib()
    f, c = C.c_int(), C.c_int()
    for world in (1, 2, 8, 9):
        covered = []
        for rank in range(world):
            assert L.smplx_shard_range(rank, world, 1024, 128, C.byref(f), C.byref(c)) == 0
            a, b = scenes.shard_range(rank, world, 1024, 128)
            assert (f.value, f.value + c.value) == (a, b)
            covered += list(range(a, b))
        assert covered == list(range(min(1024, 128 * world)))
    assert L.smplx_shard_range(3, 2, 1024, 128, C.byref(f), C.byref(c)) != 0     # rank out of range


def test_traversal_stack_is_sized_by_the_models_trees(small_cfg):
    """The sphere-tree walks of the kernels keep their stack in LDS; its size per thread comes from the model (depth of
    the trees, twice the summed depths of a checked pair), 16 bytes at least."""
    assert "#define CM_STACK_BYTES 16" in _const_header(small_cfg.robot_text)
    assert "#define CM_STACK_BYTES 24" in _const_header(scenes.with_extra_spheres(small_cfg.robot_text, 14))


@pytest.mark.parametrize("robot", ["arm7", "dual14", "mixed"])
def test_per_robot_source_compiles_for_gfx950_with_the_helper(robot, tmp_path):
    """What smplx_space_create does on the GPU box, minus the module load: header -> smplx_rtc -> code object."""
    import subprocess
    from smpl_amd import build, scenes
    text = {"arm7": scenes.arm7_robot, "dual14": scenes.dual_arm14_robot, "mixed": scenes.mixed_kinds_robot}[robot]()
    hp, op = tmp_path / "model_const.h", tmp_path / "k.hsaco"
    hp.write_text(_const_header(text))
    subprocess.check_call([build.RTC, str(hp), str(op)], timeout=600)
    code = op.read_bytes()
    assert code[:4] == b"\x7fELF"
    for k in ("k_pipe_prep", "k_pipe_setup", "k_pipe_configs", "k_pipe_finish", "k_small_batch", "k_expand", "k_state_valid",
              "k_edge_valid", "k_heuristic", "k_sphere_positions", "k_state_prep"):
        assert k.encode() in code


def test_every_source_the_kernels_include_is_embedded_and_nothing_else():
    """The per-robot build compiles kernels.hip against the sources embedded in the library (build.py writes them into
    csrc/_embedded_sources.h; rtc_compile.h hands the table to hiprtc, specialize.cpp hashes it into the cache key).  A header
    that kernels.hip reaches and the table lacks would make every per-robot build fail and fall back to the generic
    kernels: the table is the #include "..." closure of kernels.hip, found here on the test's own, and nothing else."""
    from smpl_amd import build
    capi.lib()   # builds, and with that writes the table, where there is no library yet
    found, todo = set(), ["kernels.hip"]
    while todo:
        f = todo.pop()
        if f in found:
            continue
        found.add(f)
        if f != "model_const.h":   # written for the robot at run time (model_compile.cpp model_const_header)
            text = open(os.path.join(build.CSRC, f)).read()
            todo += re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M)   # <...> includes are the toolchain's
            todo += ["model_const.h"] * len(re.findall(r'^\s*#\s*include\s+SMPLX_CONST_MODEL\b', text, re.M))
    gen = open(os.path.join(build.CSRC, build.GENERATED)).read()
    table = re.findall(r'^    \{"([^"]+)",$', gen, re.M)
    assert 'kRootSource[] =\nR"SMPLXSRC(' + open(os.path.join(build.CSRC, "kernels.hip")).read() + ')SMPLXSRC";' in gen
    assert found - {"kernels.hip"} == set(table) | {"model_const.h"}
    assert table == sorted(set(table)) and "search_kernel.h" in table    # each once, in a fixed order
    unreachable = set(os.listdir(build.CSRC)) - found
    assert {"engine.hip", "step.h", "specialize.cpp", "rtc_compile.h"} <= unreachable and not unreachable & set(table)


def test_default_is_the_forks_xy_rotation(small_cfg):
    """[FORK] manip_lattice_action_space.cpp:590-599: delta[0], delta[1] rotated by state[3] -- the reference's
    behaviour is what every config runs unless told otherwise (xy_rotate_by_var3 = 0 selects upstream smpl)."""
    from smpl_amd import scenes
    assert small_cfg.params.xy_rotate_by_var3 is True
    assert scenes.PlanningParams([scenes.DEG] * 7).xy_rotate_by_var3 is True
    for cfg in (scenes.config_mixed(n=16, nboxes=0),):
        assert cfg.params.xy_rotate_by_var3 is True
