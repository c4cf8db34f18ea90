"""host/offline_odometry --replay 1 --store_graph: the keyframe graph through the C ABI, written as the g2o text replay.write_g2o writes."""
import subprocess

import numpy as np
import pytest

from cfear_radarodometry_code_public_amd import capi, replay, synth
from test_host_cpp import build_harness

pytestmark = pytest.mark.gpu


def test_store_graph_writes_the_g2o_text_of_the_python_route(tmp_path):
    exe = build_harness()
    n = 40
    imgs, _ = synth.world_sequence(n // 2, seed=31, world_seed=55)
    imgs = np.concatenate([imgs, imgs[::-1]])
    f = tmp_path / "sweeps.u8"
    imgs.tofile(f)
    g = tmp_path / "graph.g2o"
    r = subprocess.run([exe, "--frames", str(f), "--range-res", "0.0595238", "--res", "3.0", "--submap_scan_size", "4", "--z-min", "60", "--weight_option", "4",
                        "--est_directory", str(tmp_path), "--replay", "1", "--store_graph", str(g)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "keyframes " in r.stdout and "dropped 0" in r.stdout
    # the same run through the Python layer (offline_odometry's defaults: P2L, Huber 0.1, compensation on, 1.5 m keyframes)
    p = capi.default_params(range_res=np.float32(0.0595238), z_min=60.0, k_strongest=12, min_distance=2.5, res=3.0, submap_scan_size=4, weight_intensity=1,
                            weight_opt=4, cost=1, loss=1, loss_limit=0.1, radar_ccw=0, compensate=1, min_keyframe_dist=1.5)
    ctx = capi.Context(p, 400, 3360)
    odo = ctx.odometry(1)
    odo.record_keyframes(capi.KF_NODES, 65536, 0)
    odo.replay_host(imgs)
    nodes = odo.keyframes(0)
    odo.release(); ctx.close()
    assert 15 <= len(nodes) <= 25
    e = tmp_path / "expected.g2o"
    replay.write_g2o(e, nodes)
    assert open(g).read() == open(e).read()
    back = replay.read_g2o(g)
    for fld in ("index", "prev", "pose", "t_be"):
        assert back[fld].tobytes() == nodes[fld].tobytes(), fld
    ix = np.ix_([0, 1, 5], [0, 1, 5])
    assert all(np.array_equal(np.triu(b["information"][ix]), np.triu(a["information"][ix])) for a, b in zip(nodes, back))
    # the per-sweep route has no device log: the flag is refused there, loudly
    r = subprocess.run([exe, "--frames", str(f), "--est_directory", str(tmp_path), "--store_graph", str(tmp_path / "no.g2o")], capture_output=True, text=True)
    assert r.returncode != 0 and "--replay 1" in r.stderr and not (tmp_path / "no.g2o").exists()
