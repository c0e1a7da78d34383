"""The plain model of the robot body (tests/body_ref.py) pinned by hand-derived answers, the conditions the GPU tests rely
on asserted on the model alone, and the parser-and-kinematics header (smpl_amd/csrc/robot_body.h) built by the host
compiler and compared with the model.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import body_cases as C
import body_ref as B
import kinematics_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the HalfRes lattice ----------------------------------------------------------------------------------------------
def test_half_res_discretize_table():
    """discretize.h:94-113 at res 0.01"""
    for d, want in ((-0.01, -2), (-0.005, -1), (0.0, 0), (0.005, 0), (0.01, 1)):
        assert B.discretize(d, 0.01) == want, d


def test_continuize_is_the_pivot_form_bit_for_bit():
    """i * res + 0.5 * res equals 0.5 * res + i * res (what voxelize_ref's continuize gives with the pivot 0.5 * res)"""
    import voxelize_ref as V
    for res in (0.01, 0.02, 0.0137):
        for i in range(-1000, 1001):
            assert B.continuize(i, res) == 0.5 * res + i * res == V.continuize(i, 0.5 * res, res)


def test_grid_range_where_min_plus_size_rounds_below_max():
    """voxel_grid.h:187-193: the high index is discretize(min + (max - min)).  With min = -0.3 and max = 0.03 the size is
    0.32999999999999996 and min + size = 0.02999999999999997 < max: index 2, where max itself lies in voxel 3"""
    assert 0.03 - -0.3 == 0.32999999999999996 and -0.3 + (0.03 - -0.3) < 0.03
    lo, hi = B.grid_range((-0.3, 0.0, 0.0), (0.03, 0.025, 0.0), 0.01)
    assert lo == [-31, 0, 0] and hi == [2, 2, 0] and B.discretize(0.03, 0.01) == 3
    # a triangle that reaches max has its candidates clipped to the grid's range
    cells, und = B.voxelize_mesh([(-0.3, 0.0, 0.0), (0.03, 0.0, 0.0), (0.03, 0.025, 0.0)], [(0, 1, 2)], 0.01)
    assert cells[:, 0].max() == 2 and cells[:, 0].min() >= -31


def test_right_triangle_by_hand():
    """p1 = (0.002, 0.002), p2 = (0.028, 0.002), p3 = (0.002, 0.018) in the plane z = 0.005, res 0.01, rc = 0.00866.  Candidates:
    x 0..2, y 0..1, z 0.  (0,0), (2,0), (0,1) lie within rc of a vertex (0.00424); (1,0) is inside the triangle; (1,1) is outside
    but 0.00426 from the edge p2-p3, inside its span; (2,1) is 0.0095 from that edge and 0.0133 from p2: empty."""
    cells, und = B.voxelize_mesh([(0.002, 0.002, 0.005), (0.028, 0.002, 0.005), (0.002, 0.018, 0.005)], [(0, 1, 2)], 0.01)
    assert cells.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [2, 0, 0]] and len(und) == 0
    assert np.array_equal(B.points_of(cells, 0.01)[0], [0.005, 0.005, 0.005])


def test_two_elements_are_appended_with_their_duplicates():
    text = ("link a\ngeom a box 0.03 0.02 0.04  0.0013 0.0021 0.0017  0.1 0.2 0.3\n"
            "geom a box 0.03 0.02 0.04  0.0013 0.0021 0.0017  0.1 0.2 0.3\nvoxels a 0.01\n")
    p, near, _ = B.Body(text).model_points(0)
    one = B.Body(text.replace("geom a box 0.03 0.02 0.04  0.0013 0.0021 0.0017  0.1 0.2 0.3\n", "", 1)).model_points(0)[0]
    assert len(one) > 0 and len(p) == 2 * len(one) and np.array_equal(p[:len(one)], one) and np.array_equal(p[len(one):], one)


CHAIN = """link r
link a
link b
link c
link side
link sidetip
joint ja revolute r a  0 0 0.1  0 0 0  0 0 1  -3 3
joint jb revolute a b  0 0 0.1  0 0 0  0 1 0  -3 3
joint jc revolute b c  0 0 0.1  0 0 0  1 0 0  -3 3
joint jside revolute a side  0.1 0 0  0 0 0  0 0 1  -3 3
joint jtip fixed side sidetip  0.1 0 0  0 0 0  0 0 1  0 0
voxels r 0.01
voxels a 0.01
voxels b 0.01
voxels c 0.01
voxels side 0.01
voxels sidetip 0.01
group arm c
"""


def test_descendant_dirtiness_and_group_exclusion():
    """robot_collision_state.cpp:62-96, 297-314 on a three-joint chain with a side branch; c is a group link"""
    b = B.Body(CHAIN)
    assert b.dirty == [True] * 6 and b.outside == [True, True, True, False, True, True]
    assert b.put() == [0, 1, 2, 4, 5]                 # never c; its flag stays
    assert b.dirty == [False, False, False, True, False, False]
    b.set_joint("jb", 0.0)                            # the same value dirties nothing
    assert b.put() == []
    b.set_joint("jb", 0.3)
    assert b.dirty == [False, False, True, True, False, False] and b.put() == [2]
    b.set_joint("jside", -0.2)
    assert b.put() == [4, 5]                          # through the fixed joint as well
    b.set_joint("ja", 0.1)
    assert b.put() == [1, 2, 4, 5]
    b.set_joint("jc", 0.1)
    assert b.put() == []                              # only the group link moved


# ---- the conditions of the GPU tests, on the model alone --------------------------------------------------------------
def test_shared_body_conditions():
    M = C.model()
    assert [m["link"] for m in M.models] == C.MODELS and M.outside == [m != C.GROUP_MODEL for m in range(len(C.MODELS))]
    for m in range(len(C.MODELS)):
        p, near, missing = C.model_points(m)
        if m == C.GROUP_MODEL:                        # the axis-aligned box: the project's 15 % bound
            assert 0 < near.sum() + len(missing) <= 0.15 * len(p)
        else:
            assert near.sum() == 0 and len(missing) == 0, C.MODELS[m]
    assert len(C.model_points(C.MODELS.index("tiny"))[0]) == 1
    # more than one compaction chunk (2048 mask bytes) and more than one block of the placing kernel (256 points)
    g = [g for g in M.geoms if g["link"] == "base"][0]
    v, _ = M.element_mesh(g)
    lo, hi = B.grid_range(v.min(axis=0), v.max(axis=0), 0.01)
    assert np.prod([h - l + 1 for l, h in zip(lo, hi)]) > 2048 and len(C.model_points(0)[0]) > 4 * 256
    assert len(C.strip_mesh()[1]) == 40


@pytest.mark.parametrize("second", [False, True])
def test_shared_body_placing_conditions(second):
    """no placed point within 1e-9 of a cell boundary; `edge` leaves through two faces, `far` lies wholly outside"""
    M = B.Body(C.body_text())
    if second:
        M.set_joint(*C.SECOND_Q)
    F = M.frames()
    for m, name in enumerate(C.MODELS):
        cells, margin = B.place(F[name][0], C.model_points(m)[0], C.ORIGIN, C.RES, C.DIMS)
        assert margin.min() > 1e-9, name
        inside = cells[:, 0] >= 0
        if name == "far":
            assert not inside.any()
        elif name == "edge":
            p = C.model_points(m)[0] + F[name][0][:, 3]
            assert 0 < inside.sum() < len(cells)
            assert (p[:, 0] > C.ORIGIN[0] + C.DIMS[0] * C.RES).any() and (p[:, 1] > C.ORIGIN[1] + C.DIMS[1] * C.RES).any()
        else:
            assert inside.all(), name


# ---- the header on the CPU --------------------------------------------------------------------------------------------
DRIVER = os.path.join(ROOT, "tests", "cpp", "robot_body_host_driver.cpp")


@pytest.fixture(scope="module")
def host_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("body") / "robot_body_host_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", DRIVER, "-o", exe])
    return exe


def run_driver(exe, tmp_path, text, commands=""):
    path = os.path.join(str(tmp_path), "body.txt")
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([exe, path], input=commands, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def transforms_of(line, nlinks):
    return np.array([float.fromhex(x) for x in line.split()]).reshape(nlinks, 3, 4)


def test_header_lattice_on_the_cpu(host_driver, tmp_path):
    cmds = "".join("disc %s %s\n" % (float(d).hex(), (0.01).hex()) for d in (-0.01, -0.005, 0.0, 0.005, 0.01))
    cmds += "".join("cont %d %s\n" % (i, (0.01).hex()) for i in (-1000, -1, 0, 7, 1000))
    out = run_driver(host_driver, tmp_path, "link a\n", cmds)
    assert out[0] == "ok 1 0 0" and [int(x) for x in out[1:6]] == [-2, -1, 0, 0, 1]
    assert [float.fromhex(x) for x in out[6:11]] == [B.continuize(i, 0.01) for i in (-1000, -1, 0, 7, 1000)]


def test_header_transforms_and_dirtiness_equal_the_model(host_driver, tmp_path):
    """link transforms against kinematics_ref within its BOUND (2^-46), at creation and after set_joint; dirtiness and
    the states a put places against the model"""
    M = B.Body(C.body_text())
    steps = [C.SECOND_Q, ("j1", -1.2137), ("js", 2.5137), ("jf", 0.3137), ("j1", -1.2137), ("j3", 0.7)]
    cmds = "transforms\ndirty\nput\n" + "".join("set %s %s\ndirty\nput\ntransforms\n" % (j, float(q).hex()) for j, q in steps)
    out = run_driver(host_driver, tmp_path, C.body_text(), cmds)
    assert out[0] == "ok %d %d %d" % (len(M.links), len(M.joints), len(M.models))

    def check_frames(line):
        T = transforms_of(line, len(M.links))
        F = M.frames()
        worst = max(K.error(T[i], F[l]).max() for i, l in enumerate(M.links))
        assert worst <= K.BOUND, worst

    check_frames(out[1])
    assert [int(x) for x in out[2].split()] == [int(d) for d in M.dirty]
    assert [int(x) for x in out[3].split()] == M.put()
    at = 4
    for j, q in steps:
        M.set_joint(j, q)
        assert out[at] == "set 0"
        assert [int(x) for x in out[at + 1].split()] == [int(d) for d in M.dirty], (j, q)
        assert [int(x) for x in out[at + 2].split()] == M.put(), (j, q)
        check_frames(out[at + 3])
        at += 4
    out = run_driver(host_driver, tmp_path, CHAIN, "set nosuch 0x1p0\nset jtip 0x1p0\nset ja nan\nset ja 0x1p+30\ndirty\n")
    assert out[1:5] == ["set -1"] * 4 and out[5].split() == ["1"] * 6


MALFORMED = [
    ("link a\nlink a\n", 2), ("link\n", 1), ("link a\nfrobnicate a\n", 2),
    ("link a\nlink b\njoint j planar a b 0 0 0 0 0 0 0 0 1 0 0\n", 3), ("link a\nlink b\njoint j fixed a b 0 0 0 0 0 0 0 0 1 0\n", 3),
    ("link a\nlink b\njoint j fixed a nosuch 0 0 0 0 0 0 0 0 1 0 0\n", 3), ("link a\nlink b\njoint j fixed a b 0 0 nan 0 0 0 0 0 1 0 0\n", 3),
    ("link a\nlink b\njoint j fixed a b 0 0 1e6 0 0 0 0 0 1 0 0\n", 3),
    ("link a\ngeom nosuch box 1 1 1 0 0 0 0 0 0\n", 2), ("link a\ngeom a box 1 0 1 0 0 0 0 0 0\n", 2), ("link a\ngeom a box 1 -1 1 0 0 0 0 0 0\n", 2),
    ("link a\ngeom a cone 1 1 0 0 0 0 0 0\n", 2), ("link a\ngeom a sphere inf 0 0 0 0 0 0\n", 2), ("link a\ngeom a sphere 1 0 0 0 0 0\n", 2),
    ("link a\ngeom a cylinder 1 1 0 0 0 0 0 0 7\n", 2),
    ("link a\ngeom a mesh 3 1 0 0 0 0 0 0\nv 0 0 0\nv 1 0 0\nv 0 1 0\nt 0 1 3\n", 6), ("link a\ngeom a mesh 3 1 0 0 0 0 0 0\nv 0 0 0\nv 1 0 0\nt 0 1 2\n", 5),
    ("link a\ngeom a mesh 3 1 0 0 0 0 0 0\nv 0 0 0\nv 1 0 0\nv 0 1 0\nt 0 1 -1\n", 6), ("link a\ngeom a mesh 0 1 0 0 0 0 0 0\n", 2),
    ("link a\ngeom a mesh 3 1 0 0 0 0 0 0\nv 0 0 0\nv 1 0 0\nv 0 2e6 0\nt 0 1 2\n", 5),
    ("link a\nvoxels nosuch 0.01\n", 2), ("link a\nvoxels a 0\n", 2), ("link a\nvoxels a -0.01\n", 2), ("link a\nvoxels a\n", 2),
    ("link a\nvoxels a 0.01\nvoxels a 0.02\n", 3),
    ("link a\nlink b\njoint j revolute a b 0 0 0 0 0 0 0 0 1 -1 1\nvalue nosuch 1\n", 4),
    ("link a\nlink b\njoint j revolute a b 0 0 0 0 0 0 0 0 1 -1 1\nvalue j nan\n", 4),
    ("link a\nlink b\njoint j fixed a b 0 0 0 0 0 0 0 0 1 0 0\nvalue j 1\n", 4),
    ("link a\nlink b\njoint j fixed a b 0 0 0 0 0 0 0 0 1 0 0\njoint k fixed a b 0 0 0 0 0 0 0 0 1 0 0\n", 4),
]


def test_header_refuses_malformed_texts_with_the_line(host_driver, tmp_path):
    for text, line in MALFORMED:
        out = run_driver(host_driver, tmp_path, text)
        assert out[0].startswith("error -1 line %d: " % line), (text, out)
    assert run_driver(host_driver, tmp_path, "")[0].startswith("error -1")
    cyc = "link a\nlink b\nlink c\njoint j fixed b c 0 0 0 0 0 0 0 0 1 0 0\njoint k fixed c b 0 0 0 0 0 0 0 0 1 0 0\n"
    assert run_driver(host_driver, tmp_path, cyc)[0].startswith("error -1")
    many = "".join("link l%d\n" % i for i in range(4097))
    assert run_driver(host_driver, tmp_path, many)[0].startswith("error -3 line 4097: ")


def test_header_under_the_address_and_undefined_sanitizers(tmp_path):
    """the stand-alone driver built with -fsanitize=address,undefined, on the malformed texts and on the shared body: a
    report of either sanitizer ends the program with a non-zero status"""
    exe = os.path.join(str(tmp_path), "robot_body_host_driver_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", DRIVER, "-o", exe])
    for text, _ in MALFORMED + [("", 0), ("geom", 1), ("link a\ngeom a mesh 2 1 0 0 0 0 0 0\nv 0 0 0\n", 3)]:
        assert run_driver(exe, tmp_path, text)[0].startswith("error ")
    out = run_driver(exe, tmp_path, C.body_text(), "transforms\nset j1 0x1p-1\ndirty\nput\ntransforms\n")
    assert out[0].startswith("ok ")
