"""The keyframe graph without a GPU: AddToGraph's constraint rule (odometrykeyframefuser.cpp:435-440) through the host entry against
numpy, the g2o text round trip, and the layouts of the two public structs."""
import ctypes as C

import numpy as np
import pytest


def rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def constraint_numpy(frm, to, cov):
    """AddToGraph :435-440 in numpy: t_be = Tfrom^-1 Tto, C[:3,:3] = R C[:3,:3] R^T with R the rotation of Tfrom^-1, information = C^-1"""
    def T(v):
        M = rotz(v[2])
        M[:2, 2] = v[:2]
        return M
    D = np.linalg.inv(T(np.asarray(frm, dtype=np.float64))) @ T(np.asarray(to, dtype=np.float64))
    t_be = np.array([D[0, 2], D[1, 2], np.arctan2(D[1, 0], D[0, 0])])
    Cm = np.array(cov, dtype=np.float64).reshape(6, 6).copy()
    Rm = rotz(-float(frm[2]))
    Cm[:3, :3] = Rm @ Cm[:3, :3] @ Rm.T
    return t_be, np.linalg.inv(Cm)


def registration_shaped():
    """what GetCovariance (n_scan_normal.cpp:426-430) leaves: the (x, y, yaw) block of the solver in rows / columns 0, 1, 5 - entries
    1e-6 ... 1e-3 - with the (0,5) cross term and WITHOUT (1,5), identity elsewhere"""
    c = np.eye(6)
    c[0, 0], c[1, 1], c[5, 5] = 1e-3, 4e-4, 2e-6
    c[0, 1] = c[1, 0] = 1.5e-4
    c[0, 5] = c[5, 0] = 1e-5
    return c


def sampled_shaped():
    """what estimate_cov_by_sampling (odometrykeyframefuser.cpp:261-380) leaves: a full symmetric (x, y, yaw) block in rows / columns 0, 1, 5"""
    c = np.eye(6)
    blk = np.array([[3e-3, -4e-4, 2e-5], [-4e-4, 1e-3, -6e-6], [2e-5, -6e-6, 5e-6]])
    for i, a in enumerate((0, 1, 5)):
        for j, b in enumerate((0, 1, 5)):
            c[a, b] = blk[i, j]
    return c


COVS = {"identity": np.eye(6), "registration": registration_shaped(), "sampled": sampled_shaped()}


@pytest.mark.parametrize("name", sorted(COVS))
@pytest.mark.parametrize("theta", [0.0, 0.3, -0.3, 3.1])
def test_keyframe_constraint_matches_numpy(hip_lib, name, theta):
    from cfear_radarodometry_code_public_amd import capi
    cov = COVS[name]
    assert np.linalg.cond(cov) <= 1e7
    frm, to = np.array([12.5, -3.25, theta]), np.array([11.0, -2.0, theta - 0.11])
    t_be, info = capi.keyframe_constraint(frm, to, cov)
    e_t, e_info = constraint_numpy(frm, to, cov)
    print(name, theta, "t_be err", np.max(np.abs(t_be - e_t)), "info rel err", np.max(np.abs(info - e_info)) / np.max(np.abs(e_info)))
    assert np.max(np.abs(t_be - e_t)) <= 1e-12
    assert np.max(np.abs(info - e_info)) <= 1e-6 * np.max(np.abs(e_info))
    # only the leading block turns: with a rotation the (0,5) term does not follow x into the new frame (the reference's behaviour)
    if name == "registration" and theta != 0.0:
        full = np.eye(6)
        full[:3, :3] = rotz(-theta)
        repaired = np.linalg.inv(full @ cov @ full.T)
        assert np.max(np.abs(info - repaired)) > 1e-3 * np.max(np.abs(e_info))


def test_keyframe_constraint_refuses_what_it_cannot_invert(hip_lib):
    from cfear_radarodometry_code_public_amd import capi
    with pytest.raises(capi.CfearError):
        capi.keyframe_constraint([0, 0, 0], [1, 0, 0], np.zeros((6, 6)))
    bad = np.eye(6)
    bad[2, 2] = np.nan
    with pytest.raises(capi.CfearError):
        capi.keyframe_constraint([0, 0, 0], [1, 0, 0], bad)


def hand_made_nodes():
    from cfear_radarodometry_code_public_amd import capi
    rng = np.random.default_rng(7)
    nodes = np.zeros(5, dtype=capi.KEYFRAME_NODE_DTYPE)
    for i in range(5):
        nodes[i]["index"], nodes[i]["prev"] = i, i - 1
        nodes[i]["pose"] = rng.normal(size=3) * [100.0, 100.0, 1.0]
        if i:
            nodes[i]["t_be"] = rng.normal(size=3) * [1.0, 1e-3, 1e-7]
            blk = rng.normal(size=(3, 3)) * 1e5
            blk = blk + blk.T
            for a, ia in enumerate((0, 1, 5)):
                for b, ib in enumerate((0, 1, 5)):
                    nodes[i]["information"][ia, ib] = blk[a, b]
    nodes[2]["pose"] = [1e-5, -0.0, 1e16]  # repr's two notations and a signed zero
    nodes[3]["t_be"] = [1.0 / 3.0, 5e-324, -1.7976931348623157e308]
    return nodes


def test_g2o_round_trip_is_bit_exact(tmp_path):
    from cfear_radarodometry_code_public_amd import replay
    nodes = hand_made_nodes()
    path = tmp_path / "graph.g2o"
    replay.write_g2o(path, nodes)
    lines = open(path).read().splitlines()
    assert [l.split()[0] for l in lines] == ["VERTEX_SE2"] * 5 + ["EDGE_SE2"] * 4
    assert lines[5].split()[1:3] == ["1", "0"] and len(lines[5].split()) == 12  # from the new keyframe to the previous one; dx dy dth + 6 information entries
    back = replay.read_g2o(path)
    assert back.dtype == nodes.dtype and back.tobytes() == nodes.tobytes()


def test_struct_sizes_match_the_dtypes(hip_lib):
    from cfear_radarodometry_code_public_amd import capi
    assert C.sizeof(capi.KeyframeNode) == capi.KEYFRAME_NODE_DTYPE.itemsize == 376
    assert C.sizeof(capi.KeyframeCell) == capi.KEYFRAME_CELL_DTYPE.itemsize == 72
    # (field by field, against the compiled header: test_abi_cpu.test_records_match_the_header)
