"""Skeleton graphs that parameterise the sampler: joint-correlation (adjacency) matrices and
node types.  Only the data needed to build Sigma_N and the per-type weights is kept (the
reference's skeleton classes, src/data/skeleton/kinematic/*.py, are out of scope).

Nodes are the joints without the hip/root (if_consider_hip=False, the eval setting,
configs/config_eval/task/hmp.yaml:4); the root's limbs are replaced by a hip triangle
(e.g. h36m.py:89-97).  Node types: left/right twins share a type ('LKnee'/'RKnee' ->
'Knee', kinematic/base.py:58-70).  tests/test_skeletons.py checks every table against the
adjacency, node types and names captured from the reference (tests/golden/cov_*.npz).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

# joint names WITH the root at index 0, limbs in that indexing, and the hip-triangle joints
_H36M17 = (
    ["GlobalRoot", "RHip", "RKnee", "RAnkle", "LHip", "LKnee", "LAnkle", "Torso", "Neck", "Nose", "Head",
     "LShoulder", "LElbow", "LWrist", "RShoulder", "RElbow", "RWrist"],
    [(0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (8, 14),
     (11, 12), (12, 13), (14, 15), (15, 16)],
    ("RHip", "LHip", "Torso"),
)

_AMASS22_NAMES = ["GlobalRoot", "LHip", "RHip", "Spine1", "LKnee", "RKnee", "Spine3", "LHeel", "RHeel", "Neck",
                  "LFoot", "RFoot", "BMN", "LSI", "RSI", "Head", "LShoulder", "RShoulder", "LElbow", "RElbow",
                  "LWrist", "RWrist"]
_AMASS22_LIMBS = [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (9, 14), (14, 17), (17, 19), (19, 21), (9, 13),
                  (13, 16), (16, 18), (18, 20), (0, 2), (2, 5), (5, 8), (8, 11), (0, 1), (1, 4), (4, 7), (7, 10)]


def _mano_hand(side: str, wrist: int, first: int):
    names, limbs = [], []
    for f, finger in enumerate(["index", "middle", "pinky", "ring", "thumb"]):
        base = first + 3 * f
        names += [f"{side}_{finger}{k}" for k in (1, 2, 3)]
        limbs += [(wrist, base), (base, base + 1), (base + 1, base + 2)]
    return names, limbs


_lh_n, _lh_l = _mano_hand("left", 20, 22)
_rh_n, _rh_l = _mano_hand("right", 21, 37)

_FREEMAN18 = (
    ["GlobalRoot", "LHip", "RHip", "LKnee", "RKnee", "LAnkle", "RAnkle", "Nose", "LEye", "REye", "LEar", "REar",
     "LShoulder", "RShoulder", "LElbow", "RElbow", "LWrist", "RWrist"],
    [(0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (4, 6), (0, 7), (7, 8), (7, 9), (8, 10), (9, 11), (7, 12), (7, 13),
     (12, 14), (13, 15), (14, 16), (15, 17)],
    ("RHip", "LHip", "Nose"),
)

SKELETONS: Dict[str, Tuple[List[str], List[Tuple[int, int]], Tuple[str, str, str]]] = {
    "h36m16": _H36M17,
    "amass21": (_AMASS22_NAMES, _AMASS22_LIMBS, ("LHip", "RHip", "Spine1")),
    "mano51": (_AMASS22_NAMES + _lh_n + _rh_n, _AMASS22_LIMBS + _lh_l + _rh_l, ("LHip", "RHip", "Spine1")),
    "freeman17": _FREEMAN18,
}


# hip-included variants (if_consider_hip=True, e.g. amass.py:81-83): the root joint is node 0 and
# the original limbs are kept (BASELINE config 3's "J=52" label for AMASS-MANO)
HIP_INCLUDED: Dict[str, str] = {"mano52": "mano51"}


def skeleton(key: str):
    """-> (node_names, node_limbs, adjacency (J,J) float32, node_types (J,) int64)."""
    if key in HIP_INCLUDED:
        names, limbs, _ = SKELETONS[HIP_INCLUDED[key]]
        nodes, node_limbs = list(names), [tuple(l) for l in limbs]
    else:
        names, limbs, (a, b, c) = SKELETONS[key]
        nodes = names[1:]
        idx = {n: i for i, n in enumerate(nodes)}
        node_limbs = [(idx[a], idx[b]), (idx[a], idx[c]), (idx[b], idx[c])]
        node_limbs += [(i - 1, j - 1) for i, j in limbs if i != 0 and j != 0]
    J = len(nodes)
    adj = np.zeros((J, J), dtype=np.float32)
    for i, j in node_limbs:
        adj[i, j] = adj[j, i] = 1.0
    stripped = [n[1:] if n[0] in "LR" and n[1].isupper() else n for n in nodes]
    uniq = list(dict.fromkeys(stripped))
    types = np.array([uniq.index(s) for s in stripped], dtype=np.int64)
    return nodes, node_limbs, adj, types


# ---- limb tables of the evaluation metrics ------------------------------------------------------------
# The reference's skeleton.get_limbseq() and skeleton.limb_angles_idx (if_consider_hip=False), as the
# body-realism metrics and the limb-angle MAE take them (src/config_metrics.py:18-21), in the
# reference's order: the angle chains index into limbseq.  tests/test_realism_host.py pins them to
# tests/golden/realism.npz.
def _mano_hand_limbs_by_depth(wrist: int, first: int) -> List[Tuple[int, int]]:
    """One hand's limbs as the reference lists them: the five wrist-to-finger limbs, then each finger's two."""
    bases = [first + 3 * f for f in range(5)]
    return [(wrist, b) for b in bases] + [l for b in bases for l in ((b, b + 1), (b + 1, b + 2))]


# kinematic chains of limb indices; mae compares the angle between each consecutive pair of a chain
_LIMB_ANGLE_CHAINS: Dict[str, List[List[int]]] = {
    "h36m16": [[3, 4], [0, 2, 7, 8, 9], [1, 7, 10, 12, 13], [7, 11, 14, 15]],
    "amass21": [[0, 2, 3, 4, 5, 6], [0, 3], [4, 7, 8, 9, 10], [4, 11, 12, 13, 14], [0, 15, 16, 17], [18, 19, 20]],
    "freeman17": [[0, 1, 7, 9], [0, 4, 6], [1, 8, 10], [3, 5], [2, 11, 13, 15], [1, 12, 14, 16]],
}
_LIMB_ANGLE_CHAINS["mano51"] = _LIMB_ANGLE_CHAINS["amass21"]  # the body's chains; the fingers have none


def limbseq(key: str) -> List[List[int]]:
    """The (L, 2) joint-index pairs of a skeleton's limbs (hip excluded), in the reference's order."""
    if key not in _LIMB_ANGLE_CHAINS:
        raise KeyError(f"no limb tables for skeleton {key!r} (have {sorted(_LIMB_ANGLE_CHAINS)})")
    if key == "mano51":  # the body's limbs, then per hand wrist-to-finger limbs before the finger segments
        limbs = skeleton("amass21")[1] + _mano_hand_limbs_by_depth(19, 21) + _mano_hand_limbs_by_depth(20, 36)
    else:
        limbs = skeleton(key)[1]
    return [[int(a), int(b)] for a, b in limbs]


def limb_angles_idx(key: str) -> List[List[int]]:
    """The kinematic chains of limb indices (into `limbseq(key)`) whose consecutive limbs form the
    angles of the limb-angle MAE (multimodal.py:76-102)."""
    if key not in _LIMB_ANGLE_CHAINS:
        raise KeyError(f"no limb tables for skeleton {key!r} (have {sorted(_LIMB_ANGLE_CHAINS)})")
    return [list(c) for c in _LIMB_ANGLE_CHAINS[key]]
