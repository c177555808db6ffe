#!/usr/bin/env python
"""Generates tests/golden/frame_stage.npz: what the REFERENCE does to a frame before the augmentor sees it, recorded on
synthetic frames.
  * KITTI's field-of-view flags: pcdet/utils/calibration_kitti.py Calibration.lidar_to_rect -> KittiDataset.get_fov_flag
    (pcdet/datasets/kitti/kitti_dataset.py:132-148) on every point of every KITTI-like scene, and the matrix
    np.dot(V2C.T, R0.T) the reference forms;
  * create_groundtruth_database of KittiDataset (kitti_dataset.py:224-274) and ONCEDataset (once_dataset.py:300-350), run
    into a temporary directory: the file names, every .bin's content and the dbinfos pickle;
  * box_utils.boxes3d_kitti_camera_to_lidar (box_utils.py:92-108) on float32 and float64 camera boxes.
The compiled modules are stubbed as make_augment_golden.py stubs them; points_in_boxes_cpu is that file's numpy statement
of roiaware_pool3d.cpp (margin 1e-2).  Like the other fixtures, this pins the reference's Python composition.  Scene points
stay 1e-4 m or more from every box face (enlarged by the margin), so either arithmetic decides alike.

The float32 restatement of the FOV expression lives in tests/test_frame_stage.py (fov_restatement); this generator asserts
for the fixture it writes that the restatement's flags equal the reference's on every point outside the band a float64
evaluation draws (1e-2 px around the image limits, 1e-3 m around depth 0), that the band holds at most 0.1 % of any scene,
and that the deliberately placed near-edge points are outside the band.  Only inputs and outputs are stored.

Run with the reference checkout:  python tests/golden/make_frame_stage_golden.py /path/to/reference
"""
import os
import pathlib
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_augment_golden as mag  # noqa: E402
from reference_loader import ROOT, load, module, points_in_boxes_cpu_np, q as _q, reference_root  # noqa: E402

OUT = os.path.join(HERE, "frame_stage.npz")

CALIBS = [
    dict(P2=[[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]],
         R0=[[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]],
         V2C=[[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
              [0.9998621, 0.00752379, 0.01480755, -0.2717806]]),
    dict(P2=[[707.0493, 0.0, 604.0814, 45.75831], [0.0, 707.0493, 180.5066, -0.3454157], [0.0, 0.0, 1.0, 0.004981016]],
         R0=[[0.9999128, 0.01009263, -0.008511932], [-0.01012729, 0.9999406, -0.004037671], [0.008470675, 0.004123522, 0.9999556]],
         V2C=[[0.006927964, -0.9999722, -0.002757829, -0.02457729], [-0.001162982, 0.002749836, -0.9999955, -0.06127237],
              [0.9999753, 0.006931141, -0.001143899, -0.3321029]]),
]
SHAPES = [(375, 1242), (370, 1224)]
DIMS = {"Car": (3.9, 1.6, 1.56), "Pedestrian": (0.8, 0.6, 1.73), "Cyclist": (1.76, 0.6, 1.73), "Van": (5.0, 1.9, 2.2),
        "Truck": (10.0, 2.6, 3.2), "Bus": (11.0, 2.9, 3.4)}
KITTI_USED = ["Car", "Pedestrian", "Cyclist"]


def import_reference(root):
    mag.import_reference(root)      # the stubs of make_augment_golden.py (points_in_boxes_cpu, the BEV IoU, SharedArray ...)
    calibration, box_utils, kitti, once = load(root, "pcdet", ["utils.calibration_kitti", "utils.box_utils",
                                                               "datasets.kitti.kitti_dataset", "datasets.once.once_dataset"],
                                               stubs={"datasets.once.once_toolkits": {"Octopus": None}}, real_paths=True)
    for m in (kitti, once):                 # the reference imports Path only under __main__
        if not hasattr(m, "Path"):
            m.Path = pathlib.Path
    return calibration, box_utils, kitti.KittiDataset, once.ONCEDataset


def ref_calib(calibration, c):
    return calibration.Calibration({"P2": np.array(c["P2"], np.float32), "R0": np.array(c["R0"], np.float32),
                                    "Tr_velo2cam": np.array(c["V2C"], np.float32)})


# ---- synthetic frames ---------------------------------------------------------------------------------------------------
def make_boxes(rng, names, region, zc, overlap=False, f32_centre=True):
    rows = []
    for name in names:
        d = np.array(DIMS[name]) * rng.uniform(0.9, 1.1, 3)
        ctr = np.array([rng.uniform(region[0], region[2]), rng.uniform(region[1], region[3]), zc + d[2] / 2])
        rows.append(np.concatenate([ctr, d, [rng.uniform(-np.pi, np.pi)]]))
    if overlap and len(rows) >= 2:          # the second box is pulled onto the first: they share volume
        rows[1][:2] = rows[0][:2] + [0.6, 0.3]
        rows[1][2] = rows[0][2] - rows[0][5] / 2 + rows[1][5] / 2
    b = np.array(rows, np.float64).reshape(-1, 7)
    if f32_centre and len(b):               # KITTI: rect_to_lidar returns float32 centres
        b[:, :3] = b[:, :3].astype(np.float32)
    return b


def make_scan(rng, n, boxes, per_box, c=4, behind_only=False):
    """n background points over the full circle plus per_box points inside every box."""
    ang = rng.uniform(np.pi / 2 + 0.2, 3 * np.pi / 2 - 0.2, n) if behind_only else rng.uniform(-np.pi, np.pi, n)
    r = rng.uniform(2.5, 70.0, n) ** 1.0
    p = np.zeros((n, c), np.float32)
    p[:, 0], p[:, 1] = _q(r * np.cos(ang)), _q(r * np.sin(ang))
    p[:, 2] = _q(rng.uniform(-2.2, 1.0, n))
    p[:, 3:] = _q(rng.uniform(0, 1, (n, c - 3)))
    extra = []
    for b in boxes:
        k = int(rng.integers(per_box[0], per_box[1]))
        lx, ly, lz = (rng.uniform(-0.49, 0.49, k) * b[3 + a] for a in range(3))
        co, si = np.cos(b[6]), np.sin(b[6])
        q = np.zeros((k, c), np.float32)
        q[:, 0], q[:, 1], q[:, 2] = _q(lx * co - ly * si + b[0], 1024.0), _q(lx * si + ly * co + b[1], 1024.0), _q(lz + b[2], 1024.0)
        q[:, 3:] = _q(rng.uniform(0, 1, (k, c - 3)))
        extra.append(q)
    if extra:
        p = np.concatenate([p] + extra)
        p = p[rng.permutation(len(p))]
    return p


def edge_points(calib, shape, rng):
    """Points 0.05 to 0.5 px inside and outside each of the four image limits, and 0.01 m either side of depth 0."""
    P2, R0, V2C = (np.asarray(getattr(calib, k), np.float64) for k in ("P2", "R0", "V2C"))
    H, W = shape
    targets = []
    for off in (0.05, 0.12, 0.3, 0.5):
        for sgn in (-1.0, 1.0):
            for d in (6.0, 23.0, 48.0):
                targets.append((0.0 + sgn * off, rng.uniform(40, H - 40), d))
                targets.append((W + sgn * off, rng.uniform(40, H - 40), d))
                targets.append((rng.uniform(40, W - 40), 0.0 + sgn * off, d))
                targets.append((rng.uniform(40, W - 40), H + sgn * off, d))
    for d in (0.01, -0.01):
        for k in range(6):
            targets.append((W / 2 + 20.0 * k, H / 2 - 10.0 * k, d))
    r0e, v2ce = np.eye(4), np.eye(4)
    r0e[:3, :3], v2ce[:3, :4] = R0, V2C
    inv = np.linalg.inv(r0e @ v2ce)
    out = []
    for u, v, depth in targets:
        rz = depth                                       # depth = h_2 - P2[2][3] = rz when P2[2] = (0, 0, 1, t)
        rx = (u * rz - P2[0, 2] * rz - P2[0, 3]) / P2[0, 0]
        ry = (v * rz - P2[1, 2] * rz - P2[1, 3]) / P2[1, 1]
        out.append((inv @ np.array([rx, ry, rz, 1.0]))[:3])
    p = np.zeros((len(out), 4), np.float32)
    p[:, :3] = np.array(out)
    p[:, 3] = 0.5
    return p


def main():
    tfs = module("test_frame_stage", os.path.join(ROOT, "tests", "test_frame_stage.py"))
    calibration, ref_box_utils, KittiDataset, ONCEDataset = import_reference(reference_root())
    rng = np.random.default_rng(20260117)
    calibs = [ref_calib(calibration, c) for c in CALIBS]
    data = {}

    # ---- KITTI-like frames: (points, names, calib id) -------------------------------------------------------------------
    front = (6.0, -12.0, 45.0, 12.0)
    spec = [(24000, ["Car", "Car", "Pedestrian", "Van", "Cyclist", "Car"], 0, False, False),
            (21000, ["Car", "Pedestrian", "Cyclist", "Truck", "Pedestrian"], 1, True, False),
            (26000, ["Cyclist", "Car", "Car", "Pedestrian"], 0, False, False),
            (2000, ["Car", "Pedestrian"], 1, False, True),                     # no point in view
            (3000, [], 0, False, False)]                                         # no boxes
    frames = []
    for n, names, ci, overlap, behind in spec:
        boxes = make_boxes(rng, names, (-40.0, -10.0, -8.0, 10.0) if behind else front, -1.7, overlap)
        pts = make_scan(rng, n, boxes, (40, 160), behind_only=behind)
        if len(boxes):
            pts = pts[~mag._near_face(pts.astype(np.float64), boxes.astype(np.float32).astype(np.float64), (0.0, 0.0, 0.0))]
        frames.append([pts, boxes, np.array(names, dtype="<U10"), ci])
    edge_ranges = []
    for f in (0, 1):
        e = edge_points(calibs[frames[f][3]], SHAPES[frames[f][3]], rng)
        e = e[~mag._near_face(e.astype(np.float64), frames[f][1].astype(np.float32).astype(np.float64), (0.0, 0.0, 0.0))]
        edge_ranges.append((len(frames[f][0]), len(frames[f][0]) + len(e)))
        frames[f][0] = np.concatenate([frames[f][0], e])

    # ---- the reference's FOV flags ------------------------------------------------------------------------------------------
    flags, report = [], []
    for f, (pts, boxes, names, ci) in enumerate(frames):
        calib, shape = calibs[ci], np.array(SHAPES[ci], np.int32)
        pts_rect = calib.lidar_to_rect(pts[:, 0:3])
        ref = KittiDataset.get_fov_flag(pts_rect, shape, calib)
        M = np.dot(calib.V2C.T, calib.R0.T)
        rec = tfs.calib_records_np(calib.P2, calib.R0, calib.V2C)
        assert M.dtype == np.float32 and np.array_equal(rec[:12].reshape(4, 3), M)
        mine = tfs.fov_restatement(pts, rec, shape)
        band = tfs.fov_band(pts, calib.P2, calib.R0, calib.V2C, shape)
        assert np.array_equal(mine[~band], ref[~band]), "frame %d: the restatement and the reference differ outside the band" % f
        assert band.mean() <= 1e-3, "frame %d: %.2e of the points in the band" % (f, band.mean())
        f64 = tfs.fov_float64(pts, calib.P2, calib.R0, calib.V2C, shape)[0]
        assert np.array_equal(f64[~band], ref[~band])
        if f < 2:
            s, e = edge_ranges[f]
            assert not band[s:e].any() and ref[s:e].any() and not ref[s:e].all()
        flags.append(ref)
        report.append("kitti frame %d: %d points, %d in view, %d in the band, restatement != reference on %d" % (
            f, len(pts), int(ref.sum()), int(band.sum()), int((mine != ref).sum())))
    assert flags[3].sum() == 0
    data["kitti_points"] = np.concatenate([f[0] for f in frames])
    data["kitti_offsets"] = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int64)
    data["kitti_calib_id"] = np.array([f[3] for f in frames], np.int32)
    data["kitti_edge_ranges"] = np.array(edge_ranges, np.int64)
    data["calib_P2"] = np.stack([c.P2 for c in calibs])
    data["calib_R0"] = np.stack([c.R0 for c in calibs])
    data["calib_V2C"] = np.stack([c.V2C for c in calibs])
    data["calib_M"] = np.stack([np.dot(c.V2C.T, c.R0.T) for c in calibs])
    data["image_shapes"] = np.array(SHAPES, np.int32)
    data["kitti_fov_flag"] = np.concatenate(flags)

    # ---- the reference's create_groundtruth_database, KITTI ------------------------------------------------------------------
    def run_db(cls, infos, get_lidar, **kw):
        tmp = pathlib.Path(tempfile.mkdtemp())
        with open(tmp / "infos.pkl", "wb") as fh:
            pickle.dump(infos, fh)
        fake = types.SimpleNamespace(root_path=tmp, get_lidar=get_lidar)
        cls.create_groundtruth_database(fake, info_path=tmp / "infos.pkl", split="train", **kw)
        return tmp

    ids = ["%06d" % (7 * f + 3) for f in range(len(frames))]
    infos = []
    for f, (pts, boxes, names, ci) in enumerate(frames):
        m = len(names)
        annos = {"name": names, "difficulty": rng.integers(-1, 3, m).astype(np.int32),
                 "bbox": _q(rng.uniform(0, 1200, (m, 4)), 100.0), "gt_boxes_lidar": boxes, "score": -np.ones(m)}
        infos.append({"point_cloud": {"num_features": 4, "lidar_idx": ids[f]}, "annos": annos})
    by_id = {i: f[0] for i, f in zip(ids, frames)}
    tmp = run_db(KittiDataset, infos, lambda idx: by_id[idx].copy(), used_classes=KITTI_USED)
    with open(tmp / "kitti_dbinfos_train.pkl", "rb") as fh:
        dbinfos = pickle.load(fh)
    files = sorted(os.listdir(tmp / "gt_database"))
    order = ["%s_%s_%d.bin" % (ids[f], n, i) for f, fr in enumerate(frames) for i, n in enumerate(fr[2])]
    assert sorted(order) == files
    bins = [np.fromfile(tmp / "gt_database" / name, dtype=np.float32).reshape(-1, 4) for name in order]
    assert "Van" not in dbinfos and "Truck" not in dbinfos and set(dbinfos) == set(KITTI_USED)
    owner = np.zeros(len(frames[1][0]), np.int32)
    for row in points_in_boxes_cpu_np(frames[1][0][:, :3], frames[1][1]):
        owner += row
    assert (owner >= 2).sum() >= 5, "no points in two overlapping boxes"
    data["kitti_frame_ids"] = np.array(ids)
    data["kitti_names"] = np.concatenate([f[2] for f in frames]).astype("<U10")
    data["kitti_boxes"] = np.concatenate([f[1] for f in frames]).reshape(-1, 7)
    data["kitti_box_offsets"] = np.concatenate([[0], np.cumsum([len(f[1]) for f in frames])]).astype(np.int64)
    for key in ("difficulty", "bbox", "score"):
        data["kitti_" + key] = np.concatenate([i["annos"][key] for i in infos])
    data["kitti_used_classes"] = np.array(KITTI_USED)
    data["kitti_db_files"] = np.array(order)
    data["kitti_db_points"] = np.concatenate(bins)
    data["kitti_db_point_offsets"] = np.concatenate([[0], np.cumsum([len(b) for b in bins])]).astype(np.int64)
    data["kitti_dbinfos"] = np.frombuffer(pickle.dumps(dbinfos, protocol=4), np.uint8)
    report.append("kitti database: %d objects, %d infos, counts %s, %d points in two boxes" % (
        len(order), sum(len(v) for v in dbinfos.values()), [len(b) for b in bins], int((owner >= 2).sum())))

    # ---- ONCE ----------------------------------------------------------------------------------------------------------------
    onames = ["Car", "Bus", "Pedestrian", "Cyclist", "Truck", "Car", "Pedestrian"]
    oboxes = make_boxes(rng, onames, (-35.0, -35.0, 35.0, 35.0), -1.9, overlap=True, f32_centre=False)
    opts = make_scan(rng, 8000, oboxes, (30, 120))
    opts = opts[~mag._near_face(opts.astype(np.float64), oboxes.astype(np.float32).astype(np.float64), (0.0, 0.0, 0.0))]
    oinfos = [{"frame_id": "1616343527200", "sequence_id": "000076", "annos": {"name": np.array(onames), "boxes_3d": oboxes}},
              {"frame_id": "1616343527700", "sequence_id": "000076"}]                      # a frame without annotations
    tmp = run_db(ONCEDataset, oinfos, lambda seq, fid: opts.copy(), used_classes=None)
    with open(tmp / "once_dbinfos_train.pkl", "rb") as fh:
        odb = pickle.load(fh)
    oorder = ["%s_%s_%d.bin" % (oinfos[0]["frame_id"], n, i) for i, n in enumerate(onames)]
    assert sorted(oorder) == sorted(os.listdir(tmp / "gt_database"))
    obins = [np.fromfile(tmp / "gt_database" / name, dtype=np.float32).reshape(-1, 4) for name in oorder]
    data["once_points"] = opts
    data["once_frame_id"] = np.array(oinfos[0]["frame_id"])
    data["once_names"] = np.array(onames, dtype="<U10")
    data["once_boxes"] = oboxes
    data["once_db_files"] = np.array(oorder)
    data["once_db_points"] = np.concatenate(obins)
    data["once_db_point_offsets"] = np.concatenate([[0], np.cumsum([len(b) for b in obins])]).astype(np.int64)
    data["once_dbinfos"] = np.frombuffer(pickle.dumps(odb, protocol=4), np.uint8)
    report.append("once database: %d objects, counts %s" % (len(oorder), [len(b) for b in obins]))

    # ---- boxes3d_kitti_camera_to_lidar ------------------------------------------------------------------------------------------
    cam = np.concatenate([rng.uniform(-20, 20, (9, 1)), rng.uniform(0.5, 2.5, (9, 1)), rng.uniform(3, 60, (9, 1)),
                          rng.uniform(0.5, 5, (9, 3)), rng.uniform(-np.pi, np.pi, (9, 1))], 1)
    data["cam_boxes_f32"] = cam.astype(np.float32)
    data["cam_boxes_f64"] = cam
    for ci, calib in enumerate(calibs):
        data["lidar_boxes_f32_%d" % ci] = ref_box_utils.boxes3d_kitti_camera_to_lidar(cam.astype(np.float32), calib)
        data["lidar_boxes_f64_%d" % ci] = ref_box_utils.boxes3d_kitti_camera_to_lidar(cam.copy(), calib)

    np.savez_compressed(OUT, **data)
    for r in report:
        print(r)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1500000


if __name__ == "__main__":
    main()
