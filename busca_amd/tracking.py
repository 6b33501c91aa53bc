"""The reference's `busca.tracking` surface plus every device entry point the tracker adapters call, under one name.  A facade with no logic:
each name is defined in the module of its family and re-exported here as the same object.
  track_boxes   sentinel boxes, centre / IoU distances, duplicate removal, coverage, the BUSCA recovery rule   (busca_hip.h)
  kalman        ByteTrack's Kalman filter, gating, the predicted cost of a round                               (busca_hip.h)
  kalman_store  the same filter on state that stays on the device: slots, rounds without a state copy          (busca_track.h, libbusca_track.so;
                the rounds of many sequences in one launch: busca_rounds.h, libbusca_rounds.so; a whole frame as one chain:
                busca_frame.h, libbusca_frame.so; the frames of many sequences as one chain: busca_mframe.h, libbusca_mframe.so)
  sort_store    StrongSORT's filter on state that stays on the device: NSA update, camera update, gated rounds, (busca_sort.h, libbusca_sort.so;
                Tracker._match as one staged assignment; a whole frame with the feature rows as one chain       busca_sframe.h, libbusca_sframe.so)
  assignment    linear assignment, min-cost matching, the matching cascade, associate_round, staged assignment (busca_assign.h, busca_assign_stages.h)
  appearance    cosine gallery cost, NearestNeighborDistanceMetric, StrongSORT's appearance round               (busca_appearance.h)
  ghost         GHOST's proxy distances, proxies, thresholds, cost rules and round                             (busca_ghost.h)
  ghost_motion  GHOST's linear motion model                                                                    (busca_ghost_motion.h)
  ghost_gallery GHOST's feature rings and moving-average table, the state ghost_round reads                    (busca_store.h, libbusca_store.so)
  ghost_store   GHOST's whole frame on both of those states as one chain                                       (busca_gframe.h, libbusca_gframe.so)
  ecc           camera-motion estimation for ByteTrack (u8 frames) and GHOST (float32 frames)                  (busca_hip.h, busca_ecc.h)
  crops         image crops and the host classes of the device crop pool                                       (busca_hip.h)
Host arrays or device tensors go in; every call says in its docstring what comes back and where it lives.  There is no CPU implementation.
A new family is a new module plus a re-export line here."""
import os  # noqa: F401  (np, torch, os, geometry and Slot are part of what `from busca_amd.tracking import *` gives)

import numpy as np  # noqa: F401
import torch  # noqa: F401

from . import geometry  # noqa: F401
from .appearance import (INFTY_COST, NearestNeighborDistanceMetric, appearance_cost, appearance_round, embedding_distance,  # noqa: F401
                         fuse_iou, gate_cost_matrix_mc)
from .assignment import assign_stages, associate_round, linear_assignment, linear_assignment_batch, matching_cascade, min_cost_matching  # noqa: F401
from .crop_pool import Slot  # noqa: F401
from .crops import DeviceBackedCrops, DeviceCrop, DeviceCrops, FrameHostCopy, get_bbox_crop, get_image_crops, normalize_crops  # noqa: F401
from .ecc import (GhostCameraMotion, camera_motion_compensation, find_transform_ecc, find_transform_ecc_f32, ghost_ecc_check_config,  # noqa: F401
                  ghost_motion_compensation)
from .geometry import box_extents  # noqa: F401
from .ghost import GHOST_LIMIT, ghost_check_config, ghost_cost, ghost_distance, ghost_proxies, ghost_round, ghost_thresholds  # noqa: F401
from .ghost_gallery import GhostGallery  # noqa: F401
from .ghost_motion import GhostMotion, ghost_motion_check_config  # noqa: F401
from .ghost_store import GhostFrame, GhostFrameProblem, GhostStore  # noqa: F401
from .kalman import (CHI2INV95, TRACKED, fuse_motion, gate_cost_matrix, gating_distance, multi_initiate, multi_predict, multi_update,  # noqa: F401
                     predicted_cost, tlwh_to_xyah)
from .kalman_store import ByteFrame, FrameProblem, KalmanStore, RoundProblem  # noqa: F401
from .sort_store import SortFrame, SortFrameProblem, SortStore  # noqa: F401
from .track_boxes import (center_distance, get_detection_coverage, iou_distance, is_reliable, missing_candidate_bbox, recover_with_busca,  # noqa: F401
                          remove_duplicate_stracks, warp_pos)
