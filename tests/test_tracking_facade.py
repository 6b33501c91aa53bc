"""busca_amd.tracking is a facade: every public name it ever had is still there, and is the very object its family's module defines."""
import importlib
import inspect
import os
import re

from busca_amd import _lib, geometry, tracking

# the public names of busca_amd.tracking when it was one file, by the module that defines each now
HOME = {
    "track_boxes": ["center_distance", "get_detection_coverage", "iou_distance", "is_reliable", "missing_candidate_bbox", "recover_with_busca",
                    "remove_duplicate_stracks", "warp_pos"],
    "kalman": ["CHI2INV95", "TRACKED", "fuse_motion", "gate_cost_matrix", "gating_distance", "multi_initiate", "multi_predict", "multi_update",
               "predicted_cost", "tlwh_to_xyah"],
    "assignment": ["associate_round", "linear_assignment", "linear_assignment_batch", "matching_cascade", "min_cost_matching"],
    "appearance": ["INFTY_COST", "NearestNeighborDistanceMetric", "appearance_cost", "appearance_round", "embedding_distance", "fuse_iou",
                   "gate_cost_matrix_mc"],
    "ghost": ["GHOST_LIMIT", "ghost_check_config", "ghost_cost", "ghost_distance", "ghost_proxies", "ghost_round", "ghost_thresholds"],
    "ghost_motion": ["GhostMotion", "ghost_motion_check_config"],
    "ecc": ["GhostCameraMotion", "camera_motion_compensation", "find_transform_ecc", "find_transform_ecc_f32", "ghost_ecc_check_config",
            "ghost_motion_compensation"],
    "crops": ["DeviceBackedCrops", "DeviceCrop", "DeviceCrops", "FrameHostCopy", "get_bbox_crop", "get_image_crops", "normalize_crops"],
    "geometry": ["box_extents"],
    "crop_pool": ["Slot"],
}
PLAIN_MODULES = ["geometry", "np", "os", "torch"]          # what `from busca_amd.tracking import *` (compat/busca/tracking.py) also gives


def test_every_public_name_is_the_object_of_its_module():
    names = [n for ns in HOME.values() for n in ns] + PLAIN_MODULES
    assert len(names) == len(set(names)) == 58
    assert set(names) <= {n for n in dir(tracking) if not n.startswith("_")}
    for module, ns in HOME.items():
        mod = importlib.import_module("busca_amd." + module)
        for n in ns:
            assert getattr(tracking, n) is getattr(mod, n), n
    assert tracking.geometry is geometry
    for n in ("np", "os", "torch"):
        assert inspect.ismodule(getattr(tracking, n)), n


def test_the_facade_holds_no_logic_and_geometry_does_not_import_it():
    assert not [n for n, v in vars(tracking).items() if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == tracking.__name__]
    assert not re.search(r"from\s+\.tracking\b|import\s+tracking\b", inspect.getsource(geometry))


def test_headers_lists_every_signature_table_once():
    tables = [v for k, v in vars(_lib).items() if k.endswith("SIGNATURES")]
    assert len(tables) == len(_lib.HEADERS) == 7 and all(any(t is h for h in _lib.HEADERS.values()) for t in tables)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert all(os.path.exists(os.path.join(root, "include", h)) for h in _lib.HEADERS)
