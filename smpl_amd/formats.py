"""Readers for the on-disk formats either side of the path (host side only).

* `.env` object files as `smpl_test/src/call_planner.cpp:158-207` reads them: a count, then `count` rows of
  `name x y z dim_x dim_y dim_z` (whitespace separated); anything after the counted rows is ignored.
* the `spheres_models` section of an `sbpl_collision_checking` collision-model YAML
  (`sbpl_collision_checking/src/collision_model_config.cpp`: per link a list of `{name, x, y, z, radius, priority}`),
  turned into the `sphere` lines of this repo's plain-text robot model (`DESIGN.md` section 4).
* `.mprim` files need no reader here: the C-ABI takes their text as it is (`smplx_space_create`; both the upstream and
  the fork's row format, `manip_lattice_action_space.cpp:103-195`).
"""
from __future__ import annotations


def parse_env(text: str):
    """-> [(name, (x, y, z), (dim_x, dim_y, dim_z))]; boxes are centred at (x, y, z) (`GetCollisionCube`)."""
    tok = text.split()
    if not tok:
        return []
    n = int(tok[0])             # atoi of the first token (:183)
    out = []
    k = 1
    for _ in range(n):
        if k >= len(tok):
            break
        name = tok[k]
        k += 1
        vals = []
        for _ in range(6):
            vals.append(float(tok[k]) if k < len(tok) else 0.0)   # missing numbers stay 0 as in the reference's loop
            k += 1
        out.append((name, tuple(vals[:3]), tuple(vals[3:])))
    return out


def env_objects(text: str):
    """The rows of an `.env` file as world objects: [(name, [box shape])] for `Grid.insert_object`, one box per row with
    identity rotation, centre and size as `parse_env` gives them -- what the demo builds from a scene file
    (smpl_test/src/call_planner.cpp:158-207), so that a reference scene goes through the reference's voxeliser.  Rows that
    share a name are told apart by a `#k` suffix (object ids are unique)."""
    from . import capi
    out, seen = [], {}
    for name, centre, size in parse_env(text):
        k = seen.get(name, 0)
        seen[name] = k + 1
        out.append((name if k == 0 else "%s#%d" % (name, k), [capi.box(size, capi.pose_at(centre))]))
    return out


def sphere_lines_from_collision_yaml(text: str, links=None, rename=None):
    """`sphere <link> <name> x y z radius priority` lines for the links in `links` (default: every link that lists
    spheres).  `rename` maps YAML link names to the names used in the plain-text model."""
    import yaml
    doc = yaml.safe_load(text)
    models = (doc.get("robot_collision_model") or {}).get("spheres_models") or []
    lines = []
    for m in models:
        link = m.get("link_name")
        if links is not None and link not in links:
            continue
        for sp in m.get("spheres") or []:
            lines.append("sphere %s %s %r %r %r %r %d" % ((rename or {}).get(link, link), sp["name"], float(sp["x"]), float(sp["y"]),
                                                          float(sp["z"]), float(sp["radius"]), int(sp.get("priority", 1))))
    return lines


def group_links_from_collision_yaml(text: str, group: str, urdf_xml: str | None = None):
    """Links of a collision group: nested groups first, then its chains (base -> tip, resolved through the URDF's
    parent links), then its own links, in file order (`collision_groups` of the YAML;
    sbpl_collision_checking/src/collision_model_config.cpp, robot_collision_model.cpp:517-623)."""
    import yaml
    doc = yaml.safe_load(text)
    groups = {g["name"]: g for g in ((doc.get("robot_collision_model") or {}).get("collision_groups") or [])}
    parent_of = None
    if urdf_xml is not None:
        import xml.etree.ElementTree as ET
        parent_of = {j.find("child").get("link"): j.find("parent").get("link") for j in ET.fromstring(urdf_xml).findall("joint")}

    def chain_links(base, tip):
        if parent_of is None:
            raise ValueError("group %s has a chain (%s -> %s): the URDF is needed to resolve it" % (group, base, tip))
        out, l = [], tip
        while True:
            out.append(l)
            if l == base:
                return list(reversed(out))
            if l not in parent_of:
                raise ValueError("chain tip %s is not below %s" % (tip, base))
            l = parent_of[l]

    def expand(name, seen):
        if name in seen or name not in groups:
            return []
        seen.add(name)
        g = groups[name]
        out = []
        for sub in g.get("groups") or []:
            out += expand(sub, seen)
        for c in g.get("chains") or []:
            out += chain_links(c["base"], c["tip"])
        out += [l["name"] for l in g.get("links") or []]
        return out
    links = []
    for l in expand(group, set()):
        if l not in links:
            links.append(l)
    return links


def urdf_to_robot_text(urdf_xml: str, group_name: str, group_links, planning_joints, planning_link: str,
                       sphere_lines=(), acm_pairs=(), root: str | None = None, held_at=None) -> str:
    """URDF subset -> this repo's plain-text robot model (what
    sbpl_collision_checking/src/robot_collision_model.cpp:117-286 takes from a urdf::ModelInterface):
    `<link name>`, `<joint name type>` with `<parent link>`, `<child link>`, `<origin xyz rpy>`, `<axis xyz>`,
    `<limit lower upper>`; joint types fixed / revolute / continuous / prismatic (floating and planar joints are not
    part of this path).  Only the part of the tree that leads to the group's links and the planning link is kept
    (everything else would be voxelised out-of-group geometry, which is out of scope).  Joints that are neither
    planning joints nor fixed are held at `held_at[name]` (default 0), as the reference holds the joints outside the
    planning group at their current value."""
    import xml.etree.ElementTree as ET
    rob = ET.fromstring(urdf_xml)
    if rob.tag != "robot":
        raise ValueError("not a URDF: root element is <%s>" % rob.tag)
    links = [l.get("name") for l in rob.findall("link")]
    joints = []
    for j in rob.findall("joint"):
        t = j.get("type")
        if t not in ("fixed", "revolute", "continuous", "prismatic"):
            raise ValueError("joint %s: type %s is not supported on this path" % (j.get("name"), t))
        o = j.find("origin")
        xyz = [float(x) for x in (o.get("xyz", "0 0 0") if o is not None else "0 0 0").split()]
        rpy = [float(x) for x in (o.get("rpy", "0 0 0") if o is not None else "0 0 0").split()]
        a = j.find("axis")
        axis = [float(x) for x in (a.get("xyz", "1 0 0") if a is not None else "1 0 0").split()]   # URDF default axis
        lim = j.find("limit")
        lo = float(lim.get("lower", "0")) if lim is not None else 0.0
        hi = float(lim.get("upper", "0")) if lim is not None else 0.0
        joints.append(dict(name=j.get("name"), type=t, parent=j.find("parent").get("link"), child=j.find("child").get("link"),
                           xyz=xyz, rpy=rpy, axis=axis, lo=lo, hi=hi))
    children = {j["child"] for j in joints}
    if root is None:
        roots = [l for l in links if l not in children]
        if len(roots) != 1:
            raise ValueError("cannot tell the root link: %r" % roots)
        root = roots[0]
    by_child = {j["child"]: j for j in joints}
    keep_links, keep_joints = {root}, []
    for target in list(group_links) + [planning_link]:
        chain = []
        l = target
        while l != root:
            if l not in by_child:
                raise ValueError("link %s is not connected to the root %s" % (target, root))
            chain.append(by_child[l])
            l = by_child[l]["parent"]
        for j in reversed(chain):
            if j["name"] not in [k["name"] for k in keep_joints]:
                keep_joints.append(j)
            keep_links.add(j["child"])
    held = dict(held_at or {})
    out = ["robot " + rob.get("name", "robot"), "link " + root]
    out += ["link " + l for l in links if l in keep_links and l != root]
    for j in joints:                       # file order, restricted to the kept sub-tree
        if j not in keep_joints:
            continue
        t = j["type"]
        xyz, rpy = list(j["xyz"]), j["rpy"]
        if t != "fixed" and j["name"] not in planning_joints:
            # a joint outside the planning group: frozen.  Only a zero value keeps the origin as it is.
            v = float(held.get(j["name"], 0.0))
            if v != 0.0:
                raise ValueError("joint %s is outside the planning group and held at %r: fold it into the origin first" % (j["name"], v))
            t = "fixed"
        out.append("joint %s %s %s %s  %r %r %r  %r %r %r  %r %r %r  %r %r" % (
            j["name"], t, j["parent"], j["child"], xyz[0], xyz[1], xyz[2], rpy[0], rpy[1], rpy[2],
            j["axis"][0], j["axis"][1], j["axis"][2], j["lo"], j["hi"]))
    out += [s for s in sphere_lines if s.split()[1] in keep_links]
    out.append("group %s %s" % (group_name, " ".join(group_links)))
    out += ["acm %s %s" % (a, b) for (a, b) in acm_pairs if a in keep_links and b in keep_links]
    out.append("planning_joints " + " ".join(planning_joints))
    out.append("planning_link " + planning_link)
    return "\n".join(out) + "\n"


def urdf_to_body_text(urdf_xml: str, collision_yaml_text: str, group: str, meshes=None, values=None) -> str:
    """URDF + collision-model YAML -> the body text of include/smpl_amd.h "robot body" (DESIGN.md section 20): every link
    and joint of the URDF (fixed / revolute / continuous / prismatic; planar and floating joints are not supported), a
    `geom` row per `<collision>` element of a link that has a voxel model -- `<box size>`, `<sphere radius>`,
    `<cylinder radius length>`, and `<mesh filename>` through `meshes[filename] = (vertices, triangles)`, scaled by the
    element's `scale`; a mesh that is not supplied is a ValueError, as no mesh file is loaded here -- a `voxels` row per
    entry of the YAML's `voxels_models`, the links of `group` (group_links_from_collision_yaml) and a `value` row per
    entry of `values` ({joint: position})."""
    import xml.etree.ElementTree as ET
    import yaml
    rob = ET.fromstring(urdf_xml)
    if rob.tag != "robot":
        raise ValueError("not a URDF: root element is <%s>" % rob.tag)
    doc = yaml.safe_load(collision_yaml_text)
    vox = [(m["link_name"], float(m["res"])) for m in ((doc.get("robot_collision_model") or {}).get("voxels_models") or [])]
    links = [l.get("name") for l in rob.findall("link")]
    for name, _ in vox:
        if name not in links:
            raise ValueError("voxels model on %s: the URDF has no such link" % name)
    group_links = group_links_from_collision_yaml(collision_yaml_text, group, urdf_xml)

    def six(o):
        xyz = [float(x) for x in (o.get("xyz", "0 0 0") if o is not None else "0 0 0").split()]
        rpy = [float(x) for x in (o.get("rpy", "0 0 0") if o is not None else "0 0 0").split()]
        return "%r %r %r  %r %r %r" % tuple(xyz + rpy)

    out = ["robot " + rob.get("name", "robot")] + ["link " + l for l in links]
    for j in rob.findall("joint"):
        t = j.get("type")
        if t not in ("fixed", "revolute", "continuous", "prismatic"):
            raise ValueError("joint %s: type %s is not supported" % (j.get("name"), t))
        a = j.find("axis")
        axis = [float(x) for x in (a.get("xyz", "1 0 0") if a is not None else "1 0 0").split()]   # URDF default axis
        lim = j.find("limit")
        lo = float(lim.get("lower", "0")) if lim is not None else 0.0
        hi = float(lim.get("upper", "0")) if lim is not None else 0.0
        out.append("joint %s %s %s %s  %s  %r %r %r  %r %r" % (j.get("name"), t, j.find("parent").get("link"), j.find("child").get("link"),
                                                                six(j.find("origin")), axis[0], axis[1], axis[2], lo, hi))
    with_model = {name for name, _ in vox}
    for l in rob.findall("link"):
        if l.get("name") not in with_model:
            continue
        for c in l.findall("collision"):
            g = c.find("geometry")
            shape = None if g is None else next(iter(g), None)
            o = six(c.find("origin"))
            if shape is None:
                raise ValueError("link %s: a <collision> element without geometry" % l.get("name"))
            if shape.tag == "box":
                out.append("geom %s box %s  %s" % (l.get("name"), " ".join(repr(float(x)) for x in shape.get("size").split()), o))
            elif shape.tag == "sphere":
                out.append("geom %s sphere %r  %s" % (l.get("name"), float(shape.get("radius")), o))
            elif shape.tag == "cylinder":
                out.append("geom %s cylinder %r %r  %s" % (l.get("name"), float(shape.get("radius")), float(shape.get("length")), o))
            elif shape.tag == "mesh":
                f = shape.get("filename")
                if meshes is None or f not in meshes:
                    raise ValueError("link %s: mesh %s was not supplied (mesh files are not loaded)" % (l.get("name"), f))
                s = [float(x) for x in shape.get("scale", "1 1 1").split()]
                v, t = meshes[f]
                v = [[float(p[k]) * s[k] for k in range(3)] for p in v]
                t = [[int(x) for x in q] for q in t]
                out.append("geom %s mesh %d %d  %s" % (l.get("name"), len(v), len(t), o))
                out += ["v %r %r %r" % tuple(p) for p in v] + ["t %d %d %d" % tuple(q) for q in t]
            else:
                raise ValueError("link %s: <%s> geometry is not supported" % (l.get("name"), shape.tag))
    out += ["voxels %s %r" % (name, res) for name, res in vox]
    out.append("group %s %s" % (group, " ".join(group_links)))
    out += ["value %s %r" % (n, float(q)) for n, q in (values or {}).items()]
    return "\n".join(out) + "\n"


def box_spheres(center, size, pitch, radius):
    """Spheres of one radius on a regular grid that spans a box, corners included, at most `pitch` apart (centre and size
    in a link's frame, metres): n x (x, y, z, r) for Space.attach_body.  Not the reference's mesh voxeliser
    (attached_bodies_collision_model.cpp:264-313 voxelises the shape's surface; Space.attach_object makes that model):
    a plain filled box."""
    import math
    import numpy as np
    axes = []
    for c, s in zip(center, size):
        k = int(math.ceil(s / pitch - 1e-9)) + 1 if s > 0 else 1     # a flat side: one layer
        axes.append(c - s / 2 + np.arange(k) * (s / (k - 1)) if k > 1 else np.array([float(c)]))
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return np.hstack([g, np.full((len(g), 1), float(radius))])
