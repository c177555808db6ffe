"""The host plumbing the device data stages share (pdanet_amd/stage_common.py): offsets, packing of ragged scenes, the
status column of info, and on the device the one-copy upload and the workspace of an entry point."""
import numpy as np
import pytest
import torch

from pdanet_amd import stage_common as sc


def test_offsets_of():
    for sizes, want in (([], [0]), ([0, 3, 0], [0, 0, 3, 3])):
        offs = sc.offsets_of(sizes)
        assert offs.dtype == np.int64 and offs.tolist() == want
    assert sc.offsets_of(np.array([2, 5], np.int32)).tolist() == [0, 2, 7]


def test_pack_scenes():
    rng = np.random.default_rng(3)
    scenes = [np.zeros((0, 4), np.float32), rng.normal(size=(1, 4)).astype(np.float32), rng.normal(size=(5, 4))]
    packed, offs, n_cap, C = sc.pack_scenes(scenes)
    assert packed.dtype == np.float32 and packed.shape == (6, 4) and (n_cap, C) == (5, 4)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 0, 1, 6]
    assert np.array_equal(packed[:1], scenes[1]) and np.array_equal(packed[1:], scenes[2].astype(np.float32))
    packed, offs, n_cap, C = sc.pack_scenes([np.zeros((0, 4))] * 3)
    assert packed.shape == (0, 4) and packed.dtype == np.float32 and offs.tolist() == [0, 0, 0, 0] and (n_cap, C) == (1, 4)


def test_pack_scenes_errors():
    with pytest.raises(ValueError, match="^empty batch$"):
        sc.pack_scenes([])
    for bad in ([np.zeros((2, 4)), np.zeros((2, 5))], [np.zeros((2, 4)), np.zeros(4)], [np.zeros(4)]):
        with pytest.raises(ValueError, match=r"^every scene must be \(n_i, C\) with the same C$"):
            sc.pack_scenes(bad)


def test_raise_on_status():
    rules = [(2 | 4, ": first"), (1, " second"), (8, ": third")]
    info = np.zeros((4, 4), np.int32)
    info[:, :3] = 7                                   # only the status column counts
    sc.raise_on_status(info, rules)
    sc.raise_on_status(torch.from_numpy(info), rules, "frame")
    info[3, 3] = 2
    info[2, 3] = 8 | 1                                # the lowest flagged scene, its first rule in the order of the table
    info[0, 3] = 16                                   # a bit no rule names (the voxel cap) is no error
    with pytest.raises(ValueError, match="^scene 2 second$"):
        sc.raise_on_status(info, rules)
    with pytest.raises(ValueError, match="^frame 2 second$"):
        sc.raise_on_status(torch.from_numpy(info), rules, "frame")
    info[2, 3] = 8 | 4
    with pytest.raises(ValueError, match="^scene 2: first$"):
        sc.raise_on_status(info, rules)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_upload_round_trip(pinned):
    rng = np.random.default_rng(5)
    parts = [rng.integers(-2 ** 62, 2 ** 62, 3), rng.normal(size=(6, 4)).astype(np.float32), rng.normal(size=(2, 3)),
             np.zeros(0, np.int32), rng.normal(size=1).astype(np.float32)]
    views = sc.upload(parts, torch.device("cuda"), pinned)
    assert len(views) == len(parts)
    for p, v in zip(parts, views):
        assert v.is_cuda and v.dtype == sc._TORCH_DTYPE[p.dtype] and tuple(v.shape) == p.shape
        assert v.numel() == 0 or v.data_ptr() % 16 == 0
        assert np.array_equal(v.cpu().numpy().view(np.uint8), p.view(np.uint8))
    assert sc.upload([], torch.device("cuda"), pinned) == []
    empty, = sc.upload([np.zeros((0, 7), np.float32)], torch.device("cuda"), pinned)
    assert tuple(empty.shape) == (0, 7) and empty.dtype == torch.float32


@pytest.mark.gpu
def test_workspace():
    dev = torch.device("cuda")
    with pytest.raises(ValueError, match="^batch 70000 is out of range$"):
        sc.workspace("pda_input_stage_workspace_bytes", (70000, 16), "batch 70000 is out of range", dev)
    ws = sc.workspace("pda_input_stage_workspace_bytes", (2, 300), "unused", dev)
    from pdanet_amd import _lib
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.numel() == _lib.load().pda_input_stage_workspace_bytes(2, 300) > 0
