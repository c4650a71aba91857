"""The C++ drop-in's RGB-D path: Frame::ComputeStereoFromRGBD against a mock of the entry point it calls (no device: what it
passes on, and a failing call leaving every keypoint without a depth and one error record), and on the device a Frame built from
an RGB cv::Mat and a CV_16U depth cv::Mat (tests/native_rgbd/test_rgbd_dropin.cpp) against the oracle and the independent model."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rgbd_model as M
import rgbd_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_rgbd")
f32 = np.float32


def _prog(name):
    p = os.path.join(NATIVE, name)
    assert os.path.exists(p), "tests/native_rgbd/%s is not built (run __graft_entry__.build())" % name
    return p


def test_compute_stereo_from_rgbd_against_a_mock_of_the_entry_point():
    out = subprocess.run([_prog("test_rgbd_mock")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.gpu
def test_dropin_frame_from_a_colour_image_and_a_depth_map(oracle, tmp_path):
    from orbhip.capi import KP_DTYPE
    W, H = scenes.W, scenes.H
    rgb = scenes.colourings(scenes.grey_frame())["tinted"]
    depth = scenes.depth_map()
    conv = (depth.astype(f32) * scenes.DEPTH_FACTOR).astype(f32)        # the convertTo the integrator deletes, done here in numpy
    scene, result = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    with open(scene, "wb") as f:
        f.write(struct.pack("<2i", W, H) + scenes.K_TUM1.astype(f32).tobytes() + scenes.D_TUM1.astype(f32).tobytes() +
                struct.pack("<2f", scenes.BF, scenes.DEPTH_FACTOR) + rgb.tobytes() + depth.tobytes() + conv.tobytes())
    out = subprocess.run([_prog("test_rgbd_dropin"), scene, result], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    raw = open(result, "rb").read()
    n = struct.unpack_from("<i", raw)[0]
    o = 4
    kps = np.frombuffer(raw, KP_DTYPE, n, o); o += 28 * n
    kun = np.frombuffer(raw, KP_DTYPE, n, o); o += 28 * n
    desc = np.frombuffer(raw, np.uint8, 32 * n, o).reshape(n, 32); o += 32 * n
    ur1, dz1, ur2, dz2 = (np.frombuffer(raw, f32, n, o + 4 * n * i) for i in range(4)); o += 16 * n
    lvl0 = np.frombuffer(raw, np.uint8, W * H, o).reshape(H, W)
    assert o + W * H == len(raw)
    g = M.grey(rgb, M.FMT_RGB)
    assert np.array_equal(lvl0, g), "mvImagePyramid[0] is not the grey image"
    rk, rd = oracle.Extractor(1000)(g)
    assert kps.tobytes() == rk.tobytes() and np.array_equal(desc, rd)
    xy = oracle.undistort_points(np.stack([rk["x"], rk["y"]], 1), scenes.K_TUM1, scenes.D_TUM1, scenes.K_TUM1)
    assert np.array_equal(kun["x"].view(np.uint32), xy[:, 0].astype(f32).view(np.uint32))
    mur, mdz = M.depth_at_keypoints(kps, kun, depth, scenes.DEPTH_FACTOR, scenes.BF)
    assert (mdz > 0).sum() >= 50 and (mdz < 0).sum() >= 50 and int(out.stdout.split()[2]) == (mdz > 0).sum()
    for got, want in ((ur1, mur), (ur2, mur), (dz1, mdz), (dz2, mdz)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
