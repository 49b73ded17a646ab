"""Host-side mirror of the reference's model wrapper for the hot path.

``create_model(opt)`` / ``EgoTAPAutoEncoderModel`` keep the surface ``test.py`` / ``utils/evaluate.py`` touch
(reference: model/models.py:2-17, model/egotap_autoencoder_model.py:13-350, model/base_model.py): ``set_input``,
``forward(evaluate=)``, ``evaluate(dict)``, ``set_eval_mode``, ``eval_key``, ``load_networks`` / ``save_networks``,
the ``pred_*`` attributes, ``optimize_parameters`` / ``update_learning_rate`` for training, and ``HeatmapSharedModel`` for
stage-1 training of one heatmap estimator (model/heatmap_shared_model.py).  The networks run through libegotap_hip.so; this file
is plumbing only.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
from collections import OrderedDict
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn as nn

from . import lib as _lib
from . import networks
from . import session as _session
from . import spec as _spec
from .session import ptr, stream


class _StreamTri(NamedTuple):
    """what a serving entry's triangulation launch reads with a rig per stream: the device table and the number of streams"""
    table: object
    S: int


def create_model(opt):
    name = getattr(opt, "model", "egotap_autoencoder")
    if name == "egotap_autoencoder":
        model = EgoTAPAutoEncoderModel()
    elif name == "heatmap_shared":
        model = HeatmapSharedModel()
    else:
        raise ValueError("Model [%s] not recognized." % name)
    model.initialize(opt)
    return model


class PoseTracker:
    """The serving outputs followed over time on the device (``lib.pose_track``, egotap_pose_track, ``spec.pose_track_ref``): per stream (camera rig)
    P pose rows, the root (the triangulation's t_hat) and J triangulated joints, each a One-Euro filtered 3-vector that is held over rejected frames
    and forgotten after ``params.max_hold`` of them.  ``state``: float64 [streams, P + 1 + J, 12] on the device, zeros = never seen.  Made by
    ``model.new_pose_tracker``; holds no reference to the model and takes no part in its graphs.  ``world=True``: the tracks live in a world frame
    (``lib.pose_track_world``, egotap_pose_track_world): every update then takes the headset's own pose, so a head turn no longer moves a motionless body
    through the filter; ``ortho_tol`` (None: 1e-6) is how far such a pose's matrix may be from a rotation and still count.  The state belongs to the
    frame it was made in: a tracker is one or the other for life."""

    def __init__(self, P, J, streams=1, params=None, world=False, ortho_tol=None):
        self.P, self.J, self.streams, self.world = int(P), int(J), int(streams), bool(world)
        if ortho_tol is not None and not self.world:
            raise ValueError("PoseTracker: ortho_tol goes with a world tracker (world=True); this one reads no rig pose")
        self.ortho_tol = 1e-6 if ortho_tol is None else float(ortho_tol)
        if not self.ortho_tol >= 0:
            raise ValueError(f"PoseTracker: ortho_tol must be >= 0, got {ortho_tol}")
        if self.streams < 1:
            raise ValueError(f"PoseTracker: streams must be at least 1, got {streams}")
        self.params = _spec.TrackParams() if params is None else params
        _lib.track_params_struct(self.params)              # (the field checks, now rather than at the first update)
        self._state = None
        self._unseen = None

    @property
    def state(self):
        """the device tensor (made on the current cuda device at its first use: an update makes it on the pose's device)"""
        return self._state_on(torch.device("cuda", torch.cuda.current_device()))

    def _state_on(self, dev):
        if self._state is None:
            self._state = torch.zeros((self.streams, self.P + 1 + self.J, _spec.POSE_TRACK_STATE), dtype=torch.float64, device=dev)
        return self._state

    @torch.no_grad()
    def update(self, pose, joints3d=None, frame=None, dt=None, dts=None, rig_pose=None):
        """T consecutive frames of every stream, time-major: ``pose`` [T * streams, P, 3]; ``joints3d`` [T * streams, J, 8] and ``frame``
        [T * streams, 8] the last two results of a ``return_triangulation=True`` serving call (None: no joint / no root is seen in these frames, which
        holds their tracks); ``dt`` seconds per step, or ``dts`` float32 [T] on the device -> (placed [T * streams, P, 3], tracks
        [T * streams, P + 1 + J, 8]).  ONE launch on the current stream, no synchronisation: it queues behind the serving call that made its inputs.
        A world tracker also takes ``rig_pose`` float64 [T * streams, 12] on the device, per frame the row-major 3 x 4 (R | t) of the left camera in
        the world (``spec.rig_pose``) -> (placed_world, tracks, placed_cam): the skeleton and the tracks in the world, and the skeleton back in
        each frame's own camera for an overlay; a frame whose rig pose is not a rotation within the tracker's ``ortho_tol`` is a missing sample."""
        if self.world and rig_pose is None:
            raise ValueError("PoseTracker.update: a world tracker needs rig_pose, float64 [T * streams, 12]: the left camera in the world per frame")
        if not self.world and rig_pose is not None:
            raise ValueError("PoseTracker.update: rig_pose goes with a world tracker (model.new_pose_tracker(world=True)); this one filters in the camera's frame")
        if not torch.is_tensor(pose) or pose.dim() != 3 or tuple(pose.shape[1:]) != (self.P, 3):
            raise ValueError(f"PoseTracker.update: pose is a tensor [T * streams, {self.P}, 3], got {tuple(getattr(pose, 'shape', ()))}")
        if joints3d is not None and (not torch.is_tensor(joints3d) or joints3d.dim() != 3 or joints3d.shape[1] != self.J):
            raise ValueError(f"PoseTracker.update: joints3d is a tensor [T * streams, {self.J}, 8], got {tuple(getattr(joints3d, 'shape', ()))}")
        if not pose.is_cuda:
            raise _lib.EgotapError("PoseTracker.update runs on the GPU only (no CPU fallback); move the pose to cuda")
        if joints3d is None and self.J:                    # the state keeps its joint tracks: an all-invalid record per joint
            if self._unseen is None or self._unseen.shape[0] != pose.shape[0] or self._unseen.device != pose.device:
                self._unseen = torch.zeros((pose.shape[0], self.J, 8), dtype=torch.float32, device=pose.device)
            joints3d = self._unseen
        if self.world:
            tracks, placed_world, placed_cam = _lib.pose_track_world(pose, self._state_on(pose.device), rig_pose, dt=dt, dts=dts, params=self.params, frame=frame,
                                                                     joints3d=joints3d, streams=self.streams, ortho_tol=self.ortho_tol)
            return placed_world, tracks, placed_cam
        tracks, placed = _lib.pose_track(pose, self._state_on(pose.device), dt=dt, dts=dts, params=self.params, frame=frame, joints3d=joints3d,
                                         streams=self.streams)
        return placed, tracks

    def reset(self, streams=None):
        """forget everything (None) or the named streams: their next frame is a first frame"""
        if self._state is None:
            return
        if streams is None:
            self._state.zero_()
        else:
            idx = [int(s) for s in ([streams] if isinstance(streams, int) else streams)]
            if any(not 0 <= s < self.streams for s in idx):
                raise ValueError(f"PoseTracker.reset: streams are 0 .. {self.streams - 1}, got {idx}")
            self._state[idx] = 0.0


class StereoFusion:
    """The lifted joints fused with the keypoint rays, in front of a tracker (``lib.stereo_fuse``, egotap_stereo_fuse, ``spec.stereo_fuse_ref``): per joint
    the pose row placed by t_hat is a prior, every eye that sees the joint pulls it onto its ray, one eye is enough.  Made by
    ``model.new_stereo_fusion`` from the rig of ``set_stereo_rig`` as it was at that moment; holds no reference to the model and takes no part in its
    graphs.  It keeps no state between frames."""

    def __init__(self, left, right, t, params, R=None, affine=None, min_score=_spec.STEREO_MIN_SCORE, pose_row0=0):
        self.params, self.pose_row0 = params, int(pose_row0)
        self._prm = _lib.fuse_params_struct(params)        # (the field checks, now rather than at the first update)
        self._args = _lib.stereo_triangulate_args(left, right, t, R, affine, min_score)

    @torch.no_grad()
    def update(self, pose, keypoints, frame):
        """``pose`` [B, P, 3], ``keypoints`` [B, 2, J, 4] and ``frame`` [B, 8]: what a ``return_keypoints=True, return_triangulation=True`` serving call
        returns -> (pose_fused [B, P, 3], fused [B, J, 8], stats [B, 8]).  ONE launch on the current stream, no synchronisation: it queues behind the
        serving call that made its inputs; ``tracker.update(pose_fused, joints3d, frame, ...)`` follows it."""
        return _lib._stereo_fuse_run("StereoFusion.update", self._args, self._prm, keypoints, pose, frame, self.pose_row0)


class StreamRigs:
    """The rigs of S streams behind ``model.set_stereo_rigs``: ``rigs`` a list of (left, right, t, R) and one ``min_score``.  A device table
    (``lib.stereo_rigs_table``) exists per keypoint -> calibration pixel affine a serving entry or a fusion asks for and per device, each uploaded ONCE
    at its first use; ``update`` rewrites row s of every one of them in place, in stream order, so whoever holds a table -- a captured graph, a
    ``StreamStereoFusion`` -- serves the new rig from the next launch on."""

    def __init__(self, rigs, min_score, hm_size):
        self.rigs, self.min_score, self.hm_size = list(rigs), float(min_score), int(hm_size)
        self.S = len(self.rigs)
        self._tables = {}                                   # (affine kind, device) -> (table, host)
        _lib.stereo_rigs_host([self.spec_rig(s, None) for s in range(self.S)])      # (the checks, now rather than at the first request)

    def spec_rig(self, s, affine, rig=None):
        """stream s's ``spec.StereoRig`` under ``affine``: None for the RGB / byte entries' keypoints (``spec.stereo_pixel_affine`` of the stream's own
        models), or one explicit [2, 4] for all streams"""
        left, right, t, R = self.rigs[s] if rig is None else rig
        if affine is None:
            affine = (_spec.stereo_pixel_affine(left, self.hm_size), _spec.stereo_pixel_affine(right, self.hm_size))
        return _spec.StereoRig(left, right, t, R, affine, self.min_score)

    def table(self, affine, dev):
        key = (None if affine is None else tuple(tuple(float(v) for v in row) for row in affine), str(dev))
        hit = self._tables.get(key)
        if hit is None:
            hit = self._tables[key] = _lib.stereo_rigs_table([self.spec_rig(s, key[0]) for s in range(self.S)], dev)
        return hit[0]

    def update(self, s, rig):
        if not 0 <= int(s) < self.S:
            raise ValueError(f"update_stereo_rig: stream {s} is not one of the {self.S} set by set_stereo_rigs")
        new = {key: self.spec_rig(int(s), key[0], rig) for key in self._tables}
        _lib.stereo_rig_check(self.spec_rig(int(s), None, rig), s)     # refused before any table is touched
        for key, (table, host) in self._tables.items():
            _lib.stereo_rig_write(table, host, int(s), new[key])
        self.rigs[int(s)] = rig


class StreamStereoFusion:
    """``StereoFusion`` with a rig per stream (``lib.stereo_fuse_streams``, egotap_stereo_fuse_streams): made by ``model.new_stereo_fusion`` after
    ``set_stereo_rigs``.  It reads the model's rig table, so ``model.update_stereo_rig`` is seen by the next update; one ``params`` serves all streams."""

    def __init__(self, rigs, params, affine=None, pose_row0=0):
        self.params, self.pose_row0, self.streams = params, int(pose_row0), rigs.S
        self._prm = _lib.fuse_params_struct(params)
        self._rigs, self._affine = rigs, affine

    @torch.no_grad()
    def update(self, pose, keypoints, frame):
        """as ``StereoFusion.update`` on T frames of S streams, time-major (frame b = t * S + s): frame b is fused through rig b % S.  ONE launch."""
        if not (torch.is_tensor(keypoints) and keypoints.is_cuda):
            raise _lib.EgotapError("StreamStereoFusion.update runs on the GPU only (no CPU fallback); keypoints, pose and frame on one cuda device")
        table = self._rigs.table(self._affine, keypoints.device)
        return _lib._stereo_fuse_streams_run("StreamStereoFusion.update", table, self._rigs.S, self._prm, keypoints, pose, frame, self.pose_row0)


class Skeleton:
    """A rigid skeleton and a rotation per bone behind a tracker (``lib.skeleton_fit``, egotap_skeleton_fit, ``spec.skeleton_fit_ref``): per stream the
    bone lengths are calibrated over time ((L^, n) per row, float64 [streams, P, 2] on the device, zeros = uncalibrated), re-imposed on the tracked
    positions, and each bone gets a global and a parent-relative rotation against the rig's rest pose.  Made by ``model.new_skeleton``; holds no
    reference to the model and takes no part in its graphs.  A rig with ``fixed_length`` retargets to the avatar's own proportions and keeps no state.
    With ``twist`` (a ``spec.SkeletonTwist`` of the rig, or ``set_hinges``) the bones that have a pole also roll about their own axis, from the bend
    plane of the child bone (``lib.skeleton_fit_twist``, egotap_skeleton_fit_twist); without one nothing differs from what is described above."""

    def __init__(self, P, joint_preset=None, rig=None, streams=1, params=None, twist=None):
        self.P, self.joint_preset, self.streams = int(P), joint_preset, int(streams)
        if self.streams < 1:
            raise ValueError(f"Skeleton: streams must be at least 1, got {streams}")
        self.params = _spec.SkeletonParams() if params is None else params
        _lib.skeleton_params_struct(self.params)           # (the type check, now rather than at the first update)
        self.rig = None
        self._state = None
        self._structs = None
        self.twist = None
        if twist is not None and rig is None:
            raise ValueError("Skeleton: a twist table belongs to a rig: give both, or call set_rest_pose and then set_hinges")
        if rig is not None:
            self._set_rig(rig, twist)

    def _set_rig(self, rig, twist=None):
        rig_c = _lib.skeleton_rig_struct(rig)
        if rig.P != self.P:
            raise ValueError(f"Skeleton: the rig has P = {rig.P} rows, the model's pose has {self.P}")
        structs = (rig_c, _lib.skeleton_params_struct(self.params))
        if twist is not None:
            structs += (_lib.skeleton_twist_struct(twist),)
            if twist.P != rig.P:
                raise ValueError(f"Skeleton: the twist table has P = {twist.P} rows, the rig {rig.P}")
            _spec._sk_pole_rows("Skeleton", rig, twist.pole)       # (a table made for another rig of the same size)
        self.rig, self.twist, self._structs = rig, twist, structs

    def set_rest_pose(self, pose_rows, mirror=True):
        """one frame [P, 3] (a tensor or an array) taken as the rest pose, the "stand in a T-pose" calibration (``spec.skeleton_rig_from_pose`` with the
        model's joint preset); the calibrated lengths stay"""
        if self.joint_preset is None:
            raise ValueError("Skeleton.set_rest_pose: this skeleton was made without a joint preset; give new_skeleton a rig")
        self._set_rig(_spec.skeleton_rig_from_pose(self.joint_preset, pose_rows, mirror=mirror))      # (a new rest pose: the hinges of the old one go)
        return self.rig

    def set_hinges(self, pose_rows, pole=None, bend_lo=_spec.SKELETON_BEND_LO, bend_hi=_spec.SKELETON_BEND_HI):
        """one frame [P, 3] with bent elbows and knees, the "now bend your elbows and knees" calibration (``spec.skeleton_hinges_from_pose``, then
        ``spec.skeleton_twist``); ``pole`` None: the joint preset's ``spec.SKELETON_POLE``.  From then on ``update`` also observes the twist."""
        if self.rig is None:
            raise ValueError("Skeleton.set_hinges: no rig: give model.new_skeleton a rig or call set_rest_pose(pose_rows) first")
        if pole is None:
            if self.joint_preset is None:
                raise ValueError("Skeleton.set_hinges: this skeleton was made without a joint preset; name the pole rows")
            pole = _spec.SKELETON_POLE[self.joint_preset]
        hinge = _spec.skeleton_hinges_from_pose(self.rig, pole, pose_rows, bend_hi=bend_hi)
        self._set_rig(self.rig, _spec.skeleton_twist(self.rig, pole, hinge, bend_lo=bend_lo, bend_hi=bend_hi))
        return self.twist

    @property
    def state(self):
        """the device tensor (made on the current cuda device at its first use: an update makes it on the points' device); None with fixed_length"""
        return self._state_on(torch.device("cuda", torch.cuda.current_device()))

    def _state_on(self, dev):
        if self.rig is not None and self.rig.fixed_length is not None:
            return None
        if self._state is None:
            self._state = torch.zeros((self.streams, self.P, _spec.SKELETON_STATE), dtype=torch.float64, device=dev)
        return self._state

    @torch.no_grad()
    def update(self, points, tracks=None):
        """T consecutive frames of every stream, time-major: ``points`` float32 [T * streams, P, 3], a tracker's ``placed``, ``placed_world`` or
        ``placed_cam``; ``tracks`` the tracker's records [T * streams, K, 8] (a row that the tracker has forgotten is then not seen)
        -> (rigid [T * streams, P, 4], rotations [T * streams, P, 8], lengths [T * streams, P, 2]).  ONE launch on the current stream, no
        synchronisation: it queues behind the tracker's."""
        if self.rig is None:
            raise ValueError("Skeleton.update: no rig: the project ships no avatar; give model.new_skeleton a spec.skeleton_rig(...) or call "
                             "set_rest_pose(pose_rows) with one frame to take as the rest pose")
        if not torch.is_tensor(points) or not points.is_cuda:
            raise _lib.EgotapError("Skeleton.update runs on the GPU only (no CPU fallback); points is a cuda tensor")
        if self.twist is not None:
            return _lib.skeleton_fit_twist(points, self._state_on(points.device), self.rig, self.twist, params=self.params, tracks=tracks, streams=self.streams,
                                           _structs=self._structs)
        return _lib.skeleton_fit(points, self._state_on(points.device), self.rig, params=self.params, tracks=tracks, streams=self.streams, _structs=self._structs)

    def freeze(self, on=True):
        """stop (or resume) calibrating: the lengths found so far go on being used"""
        self.params = _spec.SkeletonParams(self.params.window, self.params.min_samples, self.params.max_dev, bool(on))
        if self._structs is not None:
            self._structs[1].freeze = int(bool(on))

    def reset(self, streams=None):
        """forget the calibration of every stream (None) or of the named ones: their next frame is a first frame"""
        if self._state is None:
            return
        if streams is None:
            self._state.zero_()
        else:
            idx = [int(s) for s in ([streams] if isinstance(streams, int) else streams)]
            if any(not 0 <= s < self.streams for s in idx):
                raise ValueError(f"Skeleton.reset: streams are 0 .. {self.streams - 1}, got {idx}")
            self._state[idx] = 0.0


class Overlay:
    """What the estimators saw and found, drawn onto the frames on the device (``lib.heat_u8``, ``lib.overlay_u8``; egotap_heat_u8, egotap_overlay_u8;
    ``spec.heat_u8``, ``spec.overlay_u8``): the position heatmaps as a tinted layer, the limbs and the skeleton's bones as lines, the keypoints as discs.
    Made by ``model.new_overlay``; holds no reference to the model or its graphs.  It keeps the heat layer's tap tables per (affine, S, Hc, Wc) and
    nothing else between frames."""

    def __init__(self, n_joints, style):
        if not isinstance(style, _spec.OverlayStyle) or len(style.mark_rgba) != int(n_joints):
            raise ValueError(f"Overlay: style is a spec.OverlayStyle with one mark per heatmap joint ({n_joints}), got {style!r}")
        self.J, self.style = int(n_joints), style
        self._taps, self._styles = {}, {}

    def style_for(self, keypoints: bool, limbs: bool):
        """the style of one draw: the keypoints' marks and bones (``self.style``) and / or, per limb, two end marks that are not drawn themselves
        (alpha 0) and one bone between them in the colour of the limb's joint; the limbs' bones come after the skeleton's"""
        key = (bool(keypoints), bool(limbs))
        if key not in self._styles:
            s, J = self.style, self.J
            marks, bones, bcol = (s.mark_rgba, s.bones, s.bone_rgba) if keypoints else ((), (), ())
            if limbs:
                base = len(marks)
                marks = marks + tuple(c[:3] + (0,) for c in s.mark_rgba for _ in range(2))
                bones = bones + tuple((base + 2 * l, base + 2 * l + 1) for l in range(J))
                bcol = bcol + s.mark_rgba
            self._styles[key] = _spec.OverlayStyle(bones=bones, mark_rgba=marks, bone_rgba=bcol, r16=s.r16, w16=s.w16, min_score=s.min_score, heat_rgba=s.heat_rgba)
        return self._styles[key]

    @torch.no_grad()
    def marks(self, keypoints=None, limbs=None, eyes=2):
        """the marks of one draw, float32 [B, eyes, M, 4] (None without keypoints and limbs): the keypoint records as they are, then per limb
        (x, y) -+ length / 2 (cos phi, sin phi) with the limb's peak as the score -- computed with torch, inputs of the kernel"""
        parts = []
        if keypoints is not None:
            if not torch.is_tensor(keypoints) or keypoints.dim() != 4 or tuple(keypoints.shape[1:]) != (2, self.J, 4):
                raise ValueError(f"Overlay.draw: keypoints are a tensor [B, 2, {self.J}, 4], got {tuple(getattr(keypoints, 'shape', ()))}")
            parts.append(keypoints[:, :eyes].float())
        if limbs is not None:
            if not torch.is_tensor(limbs) or limbs.dim() != 4 or tuple(limbs.shape[1:]) != (2, self.J, 8):
                raise ValueError(f"Overlay.draw: limbs are a tensor [B, 2, {self.J}, 8], got {tuple(getattr(limbs, 'shape', ()))}")
            lb = limbs[:, :eyes].float()
            half = 0.5 * lb[..., 5]
            hx, hy = half * torch.cos(lb[..., 4]), half * torch.sin(lb[..., 4])
            zero = torch.zeros_like(hx)
            ends = torch.stack([torch.stack([lb[..., 2] - hx, lb[..., 3] - hy, lb[..., 6], zero], dim=-1),
                                torch.stack([lb[..., 2] + hx, lb[..., 3] + hy, lb[..., 6], zero], dim=-1)], dim=3)      # [B, eyes, J, 2, 4]
            parts.append(ends.reshape(lb.shape[0], lb.shape[1], 2 * self.J, 4))
        return torch.cat(parts, dim=2).contiguous() if parts else None

    def taps(self, affine, S, Hc, Wc, device, eyes=2):
        """the heat layer's tap tables, per eye (tx, ty), cached: ``affine`` None for the camera entries' keypoints (pixels of the 4S x 4S frame: x 4),
        "identity" for a canvas of the maps' own side, or per eye (ax, bx, ay, by) -- ``spec.sensor_keypoint_affine(...)`` for sensor frames"""
        if affine is None:
            affine = ((4.0, 0.0, 4.0, 0.0),) * 2
        elif isinstance(affine, str):
            if affine != "identity":
                raise ValueError(f'Overlay.draw: affine is None, "identity" or per eye (ax, bx, ay, by), got {affine!r}')
            affine = ((1.0, 0.0, 1.0, 0.0),) * 2
        affine = tuple(tuple(float(v) for v in a) for a in affine)
        if len(affine) != 2 or any(len(a) != 4 for a in affine):
            raise ValueError(f"Overlay.draw: affine is per eye (ax, bx, ay, by), two eyes, got {affine!r}")
        key = (affine[:eyes], int(S), int(Hc), int(Wc), str(device))
        if key not in self._taps:
            self._taps[key] = tuple(_lib.overlay_tap_tables(a, S, Hc, Wc, device) for a in affine[:eyes])      # (one table per eye: no two arguments alias)
        return self._taps[key]

    @torch.no_grad()
    def draw(self, left8, right8, keypoints=None, heatmaps=None, limbs=None, affine=None, out=None):
        """``left8`` / ``right8`` uint8 [B, Hc, Wc, 3] on the GPU (``right8`` None: the left eye alone) and the tensors a ``predict_pose_from_*`` call
        returned -- ``keypoints`` [B, 2, J, 4] and ``limbs`` [B, 2, J, 8] in the canvases' pixels, ``heatmaps`` [B, 6J, S, S] (its 2J position channels
        are drawn, through ``lib.heat_u8``) -> (out_left, out_right or None).  ``affine``: see ``taps``; it places the heat layer only, the keypoints
        and limbs are already canvas pixels.  ``out`` = (out_left, out_right) to write into, the canvases themselves to draw in place, None for new
        tensors.  One launch, two with heatmaps, on the current stream; no synchronisation."""
        E = 1 if right8 is None else 2
        style = self.style_for(keypoints is not None, limbs is not None)
        marks = self.marks(keypoints, limbs, E)
        heat8 = taps = None
        if heatmaps is not None:
            if not torch.is_tensor(heatmaps) or heatmaps.dim() != 4 or heatmaps.shape[1] < 2 * self.J:
                raise ValueError(f"Overlay.draw: heatmaps are a tensor [B, C >= {2 * self.J}, S, S], got {tuple(getattr(heatmaps, 'shape', ()))}")
            heat8 = _lib.heat_u8(heatmaps, 0, E * self.J, E)
            taps = self.taps(affine, heatmaps.shape[2], left8.shape[1], left8.shape[2], heat8.device, E)
        return _lib.overlay_u8(left8, right8, style, marks=marks, heat8=heat8, taps=taps, out=out)


class _Source(NamedTuple):
    """What is specific to one serving entry (predict_pose_from_rgb / _camera / _sensor / _sensor_yuv / _lens); everything else about a request is ``_serve``'s."""
    who: str                          # the entry's name, for messages
    left: torch.Tensor                # the frames as the ABI entry reads them (a graph's static inputs are clones of these) ...
    right: torch.Tensor
    B: int                            # ... and their batch
    size_query: Callable              # (h, B, chunk, &bytes): the entry's workspace size
    entries: tuple                    # the ABI functions: (base, _kp, _kpl)
    args: tuple                       # their arguments between the frames and ``pose``
    kind: tuple = ()                  # what the capture key holds besides: two sources never share a graph
    keep: tuple = ()                  # tensors a graph must keep alive besides its own buffers
    float_frames: Optional[Callable] = None       # () -> the float frames the module route reads (None: left / right are those)
    keypoint_affine: Optional[list] = None        # the module route's heatmap -> frame pixel map per eye (None: x 4)
    triangulation_affine: Optional[tuple] = None  # ``_triangulation``'s affine (None: size / (4S))
    module_route: str = "the module forwards"     # what the ``graphed=True`` refusal says this configuration runs instead


class EgoTAPAutoEncoderModel(nn.Module):
    def name(self):
        return "EgoTAP AutoEncoder model"

    def initialize(self, opt):
        self.opt = opt
        self.gpu_ids = getattr(opt, "gpu_ids", [0])
        self.isTrain = getattr(opt, "isTrain", False)
        self.save_dir = os.path.join(getattr(opt, "log_dir", "./log"), getattr(opt, "experiment_name", "experiment"))
        self.device = torch.device("cuda:{}".format(self.gpu_ids[0])) if self.gpu_ids else torch.device("cuda:0")
        self.loss_names = ["pose", "cos_sim"] if self.isTrain else []
        self.model_names = ["HeatMap", "RotHeatMap", "AutoEncoder"]
        self.visual_names, self.visual_pose_names = [], ["pred_pose", "gt_pose"]
        self.eval_key = "mpjpe"
        self.cm2mm = 10
        self.stereo = getattr(opt, "stereo", True)
        self.input_channel_scale = 2 if self.stereo else 1
        if not self.stereo:
            raise NotImplementedError("only the stereo presets are built")
        pos_opt, rot_opt = copy.deepcopy(opt), copy.deepcopy(opt)      # egotap_autoencoder_model.py:104-107
        pos_opt.num_rot_heatmap = 0
        rot_opt.num_heatmap = 0
        self.net_HeatMap = networks.HeatMap_UnrealEgo_Shared(pos_opt, getattr(opt, "model_name", "resnet18"), 2)
        self.net_RotHeatMap = networks.HeatMap_UnrealEgo_Shared(rot_opt, getattr(opt, "model_name", "resnet18"), 2)
        self.net_AutoEncoder = networks.EgoTAPAutoEncoder(opt, input_channel_scale=2)
        self.optimizers, self.schedulers = [], []
        self.to(self.device)
        self._hm_ws = None
        # --use_amp (egotap_autoencoder_model.py:21, 219, 317-323: fp16 autocast + GradScaler around the training forward / loss):
        # mapped to the reduced-precision HIP mode -- bf16 matrix-core arithmetic with fp32 accumulation and fp32 master weights.
        # bf16 keeps fp32's exponent range, so there is no loss scaling and no scaler state; evaluation stays fp32, as the
        # reference disables autocast there (options/test_options.py:15, forward(evaluate=True)).
        self.use_amp = bool(getattr(opt, "use_amp", False)) and self.isTrain
        self.amp_precision = getattr(opt, "amp_precision", "bf16")
        if self.isTrain:
            path = getattr(opt, "path_to_trained_heatmap", None)
            if path is not None:
                # egotap_autoencoder_model.py:113-126: <dir>_pos/<file> -> net_HeatMap, <dir>_<heatmap_type>/<file> -> net_RotHeatMap
                d, f = os.path.dirname(path), os.path.basename(path)
                self.load_networks(net=self.net_HeatMap, path_to_trained_weights=os.path.join(d + "_pos", f))
                self.load_networks(net=self.net_RotHeatMap,
                                   path_to_trained_weights=os.path.join(d + "_" + getattr(opt, "heatmap_type", "sin"), f))
            elif not getattr(opt, "use_gt_heatmap", False):
                # the reference would train from RGB through never-trained estimators whose parameters are not even in the
                # optimizer (egotap_autoencoder_model.py:144-148): lifting from noise.  Refuse instead of doing that silently.
                raise ValueError("training the lifting head from RGB needs --path_to_trained_heatmap (stage-1 checkpoints "
                                 "<dir>_pos/<file> and <dir>_<heatmap_type>/<file>), or --use_gt_heatmap")
            # heatmap estimators are frozen while the lifting head trains (egotap_autoencoder_model.py:127-129, 144-148)
            for n in (self.net_HeatMap, self.net_RotHeatMap):
                for prm in n.parameters():
                    prm.requires_grad = False
            from .training import EgotapAdamW
            if getattr(opt, "optimizer_type", "AdamW") != "AdamW":
                raise NotImplementedError("only AdamW (the shipped training scripts) is built")
            self.optimizer_AutoEncoder = EgotapAdamW(self.net_AutoEncoder.parameters(), lr=getattr(opt, "lr", 1e-3),
                                                     eps=getattr(opt, "opt_eps", 1e-4), weight_decay=getattr(opt, "weight_decay", 0.0))
            self.optimizers.append(self.optimizer_AutoEncoder)
            if getattr(opt, "lr_policy", None):                      # egotap_autoencoder_model.py:151-152
                from .training import get_scheduler
                self.schedulers = [get_scheduler(o, opt) for o in self.optimizers]

    # ---- data --------------------------------------------------------------------------------------------------
    def set_input(self, data):
        """Keys of dataloader/data_loader.py:166-215; only the ones the eval path reads are required."""
        self.data = data
        dev = self.device
        self.input_rgb_left = data["input_rgb_left"].to(dev, non_blocking=True)
        self.input_rgb_right = data["input_rgb_right"].to(dev, non_blocking=True)
        for k in ("gt_heatmap_left", "gt_heatmap_right", "gt_limb_heatmap_left", "gt_limb_heatmap_right"):
            setattr(self, k, data[k].to(dev, non_blocking=True) if k in data else None)
        self.gt_pose = data["gt_local_pose"].to(dev, non_blocking=True) if "gt_local_pose" in data else None
        if self.gt_heatmap_left is None and "gt_camera_2d_left" in data and getattr(self.opt, "use_gt_heatmap", False):
            # joints instead of rendered heatmaps: synthesise them on the device (the data loader's per-frame CPU work,
            # dataloader/data_loader.py:76-215); gt_local_pose_full = all J+1 joints incl. the root, for the limb directions
            full = data.get("gt_local_pose_full", data["gt_local_pose"]).to(dev)
            syn = _lib.synth_heatmaps(data["gt_camera_2d_left"].to(dev), data["gt_camera_2d_right"].to(dev), full,
                                      self.opt.joint_preset, self.net_AutoEncoder.preset.hm_size)
            for k in ("gt_heatmap_left", "gt_heatmap_right", "gt_limb_heatmap_left", "gt_limb_heatmap_right"):
                setattr(self, k, syn[k])
            self._gt_cat = syn["cat"]

    # ---- forward -----------------------------------------------------------------------------------------------
    def _estimator_bn_modes(self):
        """(position net, limb net) -> True where the estimator normalises with BATCH statistics.  The reference's estimators are plain
        sub-modules of the wrapper: they run in whatever mode their `.training` flag says.  train.py:91 `model.train()` therefore
        leaves the FROZEN estimators' BatchNorm2d on batch statistics, running statistics drifting, while the head trains
        (egotap_autoencoder_model.py:127-129 freezes parameters only), and set_eval_mode() (:325-327) switches net_HeatMap but not
        net_RotHeatMap.  That is the default here too (pinned by tests/golden/wrapper_step_rgb_ue_b2.npz, the reference wrapper's own
        run).  opt.frozen_heatmap_bn_eval = True is the opt-out: folded running-statistics BatchNorm in both estimators whatever
        their mode (what the stage-1 checkpoints were validated with; frames then stay independent and large batches run in chunks on
        the bf16 channels-last kernels)."""
        if getattr(self.opt, "frozen_heatmap_bn_eval", False):
            return False, False
        return bool(self.net_HeatMap.training), bool(self.net_RotHeatMap.training)

    @staticmethod
    def _adjacent_channel_slices(parts):
        """True when the tensors are consecutive dim-1 slices of ONE contiguous fp32 CUDA [B, C, S, S] tensor that holds nothing else per frame"""
        a = parts[0]
        if not all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in parts):
            return False
        S2 = a.shape[2] * a.shape[3]
        ctot = sum(t.shape[1] for t in parts)
        want_stride = (ctot * S2, S2, a.shape[3], 1)
        off = a.storage_offset()
        base = a.untyped_storage().data_ptr()
        for t in parts:
            if t.untyped_storage().data_ptr() != base or tuple(t.stride()) != want_stride or t.shape[0] != a.shape[0] or tuple(t.shape[2:]) != tuple(a.shape[2:]) \
                    or t.storage_offset() != off:
                return False
            off += t.shape[1] * S2
        return True

    def forward_heatmap(self):
        p = self.net_AutoEncoder.preset
        J = p.n_joints_hm
        if getattr(self.opt, "use_gt_heatmap", False):
            parts = (self.gt_heatmap_left, self.gt_heatmap_right, self.gt_limb_heatmap_left, self.gt_limb_heatmap_right)
            if getattr(self, "_gt_cat", None) is not None and self.gt_heatmap_left.data_ptr() == self._gt_cat.data_ptr():
                cat = self._gt_cat                     # synthesised in place in the head's layout: no torch.cat
            elif self._adjacent_channel_slices(parts):
                # [r5] the four maps already ARE consecutive channel slices of one fp32 [B, 6J, S, S] tensor (a loader that renders into the
                # head's layout, bench.py's resident inputs): the concatenation of egotap_autoencoder_model.py:195-216 is that tensor -- a view,
                # not a 1.4 GB copy per 1024-frame step
                a = parts[0]
                cat = a.as_strided((a.shape[0], sum(t.shape[1] for t in parts), a.shape[2], a.shape[3]), a.stride(), a.storage_offset())
            else:
                cat = torch.cat(parts, dim=1).float().contiguous()
        else:
            left = self.input_rgb_left.float().contiguous()
            right = self.input_rgb_right.float().contiguous()
            B = left.shape[0]
            cat = torch.empty((B, p.in_channels, p.hm_size, p.hm_size), dtype=torch.float32, device=left.device)
            bn_batch = self._estimator_bn_modes()
            for net, batch_stats in ((self.net_HeatMap, bn_batch[0]), (self.net_RotHeatMap, bn_batch[1])):
                if batch_stats and not getattr(net, "bottleneck", False):      # refuse before either estimator launches anything
                    _spec.hm_check_batch_stats_side(net.hm_size, "a frozen estimator in train mode (batch-statistics BatchNorm; "
                                                    "model.eval() / set_eval_mode() or --frozen_heatmap_bn_eval select the eval forward)")
            # position net: channels [0, 2J) (left | right), limb net: [2J, 6J) (left cos, sin | right cos, sin)
            for net, c0, cn, batch_stats in ((self.net_HeatMap, 0, 2 * J, bn_batch[0]), (self.net_RotHeatMap, 2 * J, 4 * J, bn_batch[1])):
                if batch_stats and getattr(net, "bottleneck", False):
                    # resnet50 / resnet101 estimators have no batch-statistics forward: keep the reference command line running on the
                    # eval-mode (folded running statistics) forward below and say so once -- the deviation is exactly what
                    # --frozen_heatmap_bn_eval selects explicitly
                    if not getattr(self, "_warned_bottleneck_bn", False):
                        import warnings
                        warnings.warn(f"frozen {net.model_name} estimators run with running-statistics BatchNorm although the wrapper is in train mode "
                                      "(train.py:91 would use batch statistics; only resnet18 / resnet34 have that forward here): same as "
                                      "--frozen_heatmap_bn_eval; running statistics are not updated", RuntimeWarning, stacklevel=3)
                        self._warned_bottleneck_bn = True
                    batch_stats = False
                if batch_stats and net.precision == "bf16" and B >= 2:
                    # [r5] --use_amp: batch-statistics BatchNorm on the bf16 channels-last kernels (egotap_hm_forward_bnbatch) -- the backbone over
                    # the whole batch (the statistics couple its frames), the BatchNorm-free decoder in hm_chunk pieces, straight into the
                    # head's input slice; one scratch shared by both estimators
                    chunk = min(B, int(getattr(self.opt, "hm_chunk", 256)))
                    net.forward_bnbatch_into(left, right, cat, c0, chunk=chunk, workspace=self.net_HeatMap.bnbatch_workspace(B, chunk, left.device))
                elif batch_stats:
                    # fp32 / bf16x3: the stage-1 train-mode forward without a graph (conv_f32 / conv_bf16 kernels + bn2d_fwd), whole batch
                    from .hm_training import hm_train_forward_nograd
                    cat[:, c0:c0 + cn] = hm_train_forward_nograd(net, left, right)
                else:
                    # eval-mode estimators treat frames independently: walk a large batch in chunks so that the U-Net scratch stays
                    # at the chunk's size (B = 1024 from RGB, BASELINE config 3); one scratch shared by both estimators
                    was = net.training
                    net.eval()
                    try:
                        chunk = min(B, int(getattr(self.opt, "hm_chunk", 256)))
                        ws = None if net.bottleneck else self.net_HeatMap._workspace(chunk, left.device)   # (Bottleneck nets allocate per call)
                        for lo in range(0, B, chunk):
                            hi = min(B, lo + chunk)
                            net.forward_into(left[lo:hi], right[lo:hi], cat[lo:hi], c0, workspace=ws)
                    finally:
                        net.train(was)
        self.pred_heatmap_cat = cat
        self.pred_heatmap_left, self.pred_heatmap_right = cat[:, :J], cat[:, J:2 * J]
        self.pred_limb_heatmap_left, self.pred_limb_heatmap_right = cat[:, 2 * J:4 * J], cat[:, 4 * J:]

    def forward(self, evaluate=False):
        with torch.no_grad():                      # the estimators never train here (egotap_autoencoder_model.py:179 with train_heatmap False)
            self.forward_heatmap()
        if self.net_AutoEncoder.training:          # (evaluate only switches autocast off in the reference: egotap_autoencoder_model.py:219)
            from .training import lift_train_forward
            self.pred_pose = lift_train_forward(self.net_AutoEncoder, self.pred_heatmap_cat)
            _, self.pred_rot, self.pred_indep_pos, rec = self.net_AutoEncoder._zero_outputs(self.pred_heatmap_cat.shape[0], self.pred_pose.device)
        else:
            self.pred_pose, self.pred_rot, self.pred_indep_pos, rec = self.net_AutoEncoder(
                self.pred_heatmap_cat, self.input_rgb_left, self.input_rgb_right)
        J = self.net_AutoEncoder.preset.n_joints_hm
        self.pred_heatmap_rec_cat = rec
        self.pred_heatmap_left_rec, self.pred_heatmap_right_rec = rec[:, :J], rec[:, J:2 * J]
        self.pred_limb_heatmap_left_rec, self.pred_limb_heatmap_right_rec = rec[:, 2 * J:4 * J], rec[:, 4 * J:]

    def backward_AutoEncoder(self):
        from .training import PoseLossFn
        lam_m = getattr(self.opt, "lambda_mpjpe", 0.1)
        lam_c = getattr(self.opt, "lambda_cos_sim", -0.01)
        both = PoseLossFn.apply(self.net_AutoEncoder, self.pred_pose, self.gt_pose, lam_m, lam_c)
        self.loss_pose, self.loss_cos_sim = both[0], both[1]
        self.loss_total = self.loss_total + both.sum()

    def optimize_parameters(self):
        """One step of egotap_autoencoder_model.py:299-323: forward, loss, backward, AdamW -- all on HIP kernels (fp32, or the
        bf16 mode under --use_amp; no GradScaler: bf16 has fp32's exponent range)."""
        if not self.isTrain:
            raise RuntimeError("optimize_parameters() needs a model created with opt.isTrain = True")
        self.net_AutoEncoder.train()
        if self.use_amp:           # --use_amp: reduced-precision training arithmetic (opt.amp_precision, default "bf16"); the reference's
            # autocast spans the frozen estimators' forward too (egotap_autoencoder_model.py:219).  The requested mode is set
            # explicitly: whatever a caller (or evaluate()) left on the networks, the step runs in opt.amp_precision.
            # The mode is opt.amp_precision -- unless the caller chose a reduced mode for the whole model explicitly with
            # model.set_precision("bf16x3" | "bf16"): that choice wins over the flag's default and is kept from step to step.
            want = getattr(self, "_explicit_precision", None) or self.amp_precision
            for n in (self.net_AutoEncoder, self.net_HeatMap, self.net_RotHeatMap):
                if getattr(n, "bottleneck", False):
                    continue                                     # resnet50 / resnet101 estimators run in fp32 only (frozen here anyway)
                if n.precision != want:
                    n.set_precision(want)
        for o in self.optimizers:
            o.zero_grad()
        self.forward()
        self.loss_total = 0.0
        self.backward_AutoEncoder()
        self.loss_total.backward()          # data parallel: the gradient all-reduce runs INSIDE the backward, bucket by bucket, overlapped
        for o in self.optimizers:          # with it (parallel.GradReducer on the flat gradient arena); the gradients arrive averaged
            o.step()

    def set_precision(self, mode: str = "f32"):
        """f32 (default) | bf16x3 | bf16 for the three networks (the reference's analogous switch is --use_amp).
        Under --use_amp the training step runs in opt.amp_precision; an explicit set_precision("bf16x3" | "bf16") on the model overrides
        that default for every following step, set_precision("f32") hands the choice back to the flag (a training step under --use_amp
        is never fp32: the reference's is not either)."""
        self._explicit_precision = mode if mode != "f32" else None
        for n in (self.net_HeatMap, self.net_RotHeatMap, self.net_AutoEncoder):
            if getattr(n, "bottleneck", False) and mode != "f32":
                continue                                         # resnet50 / resnet101 estimators: fp32 only
            n.set_precision(mode)
        return self

    def freeze_weights(self, batch: int = 1):
        """Frozen-weight serving (networks._FrozenWeights): freeze every network that can be frozen as it stands -- "bf16" precision, eval mode, a
        geometry with prepared weights -- and skip the others BY NAME: returns {model name: reason} for the skipped ones.  ``batch`` is the batch
        the estimators' packed layout is built for (the chunk forward_heatmap() walks: min(batch size, opt.hm_chunk)).  A training step
        afterwards works unchanged: optimize_parameters() puts the head in train mode, which unfreezes it.  Note that evaluate() under
        --use_amp switches the networks to fp32 and back, which unfreezes them as every set_precision does."""
        skipped = OrderedDict()
        for name in self.model_names:
            net = getattr(self, "net_" + name)
            try:
                if isinstance(net, networks.HeatMap_UnrealEgo_Shared):
                    net.freeze_weights(batch)
                else:
                    net.freeze_weights()
            except _lib.EgotapError as e:
                skipped[name] = str(e)
        return skipped

    def unfreeze_weights(self):
        for name in self.model_names:
            getattr(self, "net_" + name).unfreeze_weights()
        return self

    def set_eval_mode(self):
        """egotap_autoencoder_model.py:325-327: the head and the POSITION estimator; net_RotHeatMap keeps its mode, exactly as in the
        reference (every caller there runs model.eval() first: utils/evaluate.py:93, 150).  opt.frozen_heatmap_bn_eval makes the
        estimators' mode irrelevant."""
        self.net_AutoEncoder.eval()
        self.net_HeatMap.eval()

    def evaluate(self, runnning_average_dict):
        self.set_eval_mode()
        with torch.no_grad():
            nets = (self.net_AutoEncoder, self.net_HeatMap, self.net_RotHeatMap)
            prec = [n.precision for n in nets]
            try:
                if self.use_amp:
                    for n, q in zip(nets, prec):
                        if q != "f32":
                            n.set_precision("f32")               # autocast is off in evaluation (forward(evaluate=True))
                self.forward(evaluate=True)
            finally:                                             # an exception in the forward must not leave training in fp32
                if self.use_amp:
                    for n, q in zip(nets, prec):
                        if n.precision != q:
                            n.set_precision(q)
            # one fused launch: per-sample MPJPE + Procrustes-aligned MPJPE.
            # batches of 2 or 3 frames: the reference's batch_compute_similarity_transform_torch aligns the wrong axes there
            # (utils/util.py:337) and test.py prints that number; reproduced by default, opt.pa_mpjpe_reference_batch_axes = False
            # gives every frame the PA-MPJPE it has in any other batch
            err, pa = _lib.pose_metrics(self.pred_pose, self.gt_pose,
                                        reference_batch_axes=bool(getattr(self.opt, "pa_mpjpe_reference_batch_axes", True)))
            err, pa = (err * self.cm2mm).cpu(), (pa * self.cm2mm).cpu()      # one device->host copy, not one per sample
        for i in range(self.pred_pose.shape[0]):
            runnning_average_dict.update(dict(mpjpe=err[i], pa_mpjpe=pa[i]))
        return self.pred_pose, self.pred_heatmap_cat, runnning_average_dict

    # ---- serving: stereo RGB -> pose in one call (egotap.h egotap_predict_pose_rgb) ------------------------------
    def _rgb_one_call_refusal(self):
        """None when the three networks can share ONE library handle (egotap_predict_pose_rgb), else the reason they cannot"""
        nets = (self.net_HeatMap, self.net_RotHeatMap, self.net_AutoEncoder)
        for n in nets[:2]:
            if n.bottleneck:
                return f"{n.model_name} estimators have no one-call forward (Bottleneck blocks are composed on the host)"
        if nets[0].blocks != nets[1].blocks:
            return "the two estimators have different backbones"
        prec = {n.precision for n in nets}
        if len(prec) != 1:
            return f"the three networks run in different precisions {sorted(prec)} (a handle has one)"
        return None

    def _rgb_state(self, dev):
        """The serving handle: all three networks' tensors bound to ONE egotap handle, in the networks' precision, with the head's bf16 scratch
        buffers attached and -- for every network that is frozen -- that network's own arena (prepared once more through this handle: the same
        kernel writes the same bytes).  Nothing here changes a network: flags, precision and frozen state are read, never set."""
        lib = _lib.load()
        lift, pos, rot = self.net_AutoEncoder, self.net_HeatMap, self.net_RotHeatMap
        nets = ((_lib.NET_LIFT, lift), (_lib.NET_HM_POS, pos), (_lib.NET_HM_ROT, rot))
        st = self.__dict__.get("_rgb")
        if st is None:
            st = self._rgb = _session.Serving(_session.Handle(lift.preset, hm_blocks=pos.blocks, shared_device=lift._shared_device))
        h = st.handle.h
        if any([st.handle.bind(net_id, n._bound_tensors(), dev) for net_id, n in nets]):      # (a list: all three, whichever moved)
            st.frozen = [None, None, None]                 # a moved tensor unfreezes its network inside the library
        prec = lift.precision
        if prec != st.precision:
            _lib.check(lib.egotap_set_precision(h, _lib.PRECISIONS[prec]))
            st.precision, st.frozen, st.wscratch, st.ascratch = prec, [None, None, None], None, None
            _lib.check(lib.egotap_set_weight_scratch(h, None, 0))
            _lib.check(lib.egotap_set_act_scratch(h, None, 0))
        if prec == "bf16":
            wsc = getattr(lift, "_wscratch", None)
            if wsc is not None and wsc.device == dev and st.wscratch is not wsc:
                _lib.check(lib.egotap_set_weight_scratch(h, ptr(wsc), wsc.numel()))
                st.wscratch = wsc
        for i, (net_id, n) in enumerate(nets):
            if n.weights_frozen:
                n._bind(dev)
                n._frozen_check(dev)           # stale prepared weights are redone by their owner, into the arena this handle reads too
                key = (n._frozen_arena.data_ptr(), getattr(n, "_frozen_batch", 0))
                if st.frozen[i] != key:
                    arena = n._frozen_arena
                    if n is lift:
                        _lib.check(lib.egotap_lift_freeze(h, ptr(arena), arena.numel(), stream(dev)))
                    else:
                        _lib.check(lib.egotap_hm_freeze(h, net_id, n._frozen_batch, ptr(arena), arena.numel(), stream(dev)))
                    st.frozen[i] = key
            elif st.frozen[i] is not None:
                _lib.check(lib.egotap_lift_unfreeze(h) if n is lift else lib.egotap_hm_unfreeze(h, net_id))
                st.frozen[i] = None
        return st

    def _rgb_attach_act_scratch(self, st, B, dev):
        lift = self.net_AutoEncoder
        lift._act_scratch(B, dev)              # (bf16 below the bf16-storage route's batch only; grown with the batch)
        asc = getattr(lift, "_ascratch", None)
        if st.precision == "bf16" and asc is not None and st.ascratch is not asc:
            _lib.check(_lib.load().egotap_set_act_scratch(st.handle.h, ptr(asc), asc.numel()))
            st.ascratch = asc

    def rgb_form(self):
        """how the last predict_pose_from_rgb call handed the heatmaps to the head (egotap_debug.h): "heatmaps" (fp32, returned), "scratch"
        (fp32, inside the workspace), "handoff" (conv_heatmap wrote the head's bf16 operand; no fp32 heatmaps), or "none" """
        st = self.__dict__.get("_rgb")
        if st is None:
            return "none"
        form = C.c_int()
        _lib.check(_lib.load().egotap_debug_predict_pose_rgb_form(st.handle.h, C.byref(form)))
        return _lib.RGB_FORMS[form.value]

    def set_stereo_rig(self, left, right, t, R=None, min_score=_spec.STEREO_MIN_SCORE):
        """The stereo rig ``return_triangulation`` uses: ``left`` / ``right`` the two cameras' fisheye models (``spec.OcamModel``, or paths of the
        reference's fisheye.calibration_{side}.json), ``t`` (3) the right camera's origin and ``R`` (3 x 3, None: identity -- the reference's data has
        parallel camera axes) its axes in the left camera's frame, in the pose's units: the reference's gt_pelvis_left - gt_pelvis_right.  ``min_score``:
        the keypoint score below which a joint is not triangulated (target maps peak at 1 in view and are zero otherwise: 0.5 is halfway)."""
        left, right = (m if isinstance(m, _spec.OcamModel) else _spec.ocam_from_json(m) for m in (left, right))
        t = tuple(float(v) for v in t)
        R = None if R is None else tuple(tuple(float(v) for v in row) for row in R)
        _lib.stereo_triangulate_args(left, right, t, R, None, min_score)           # (the shape checks, now rather than at the first request)
        self._stereo_rig = (left, right, t, R, float(min_score))
        self._stereo_rigs = None                            # the later of set_stereo_rig / set_stereo_rigs wins

    @staticmethod
    def _parsed_rig(who, rig):
        if not (isinstance(rig, (tuple, list)) and len(rig) in (3, 4)):
            raise ValueError(f"{who}: a rig is (left, right, t) or (left, right, t, R), got {rig!r}")
        left, right = (m if isinstance(m, _spec.OcamModel) else _spec.ocam_from_json(m) for m in rig[:2])
        t = tuple(float(v) for v in rig[2])
        R = None if len(rig) == 3 or rig[3] is None else tuple(tuple(float(v) for v in row) for row in rig[3])
        return left, right, t, R

    def set_stereo_rigs(self, rigs, min_score=_spec.STEREO_MIN_SCORE):
        """A camera rig per stream for ``return_triangulation`` and ``new_stereo_fusion``: ``rigs`` a list of (left, right, t, R=None) as
        ``set_stereo_rig`` takes them, stream 0 first; a serving call then carries T frames of S = len(rigs) streams, time-major (frame b = t * S + s,
        as the trackers take them), B a multiple of S, and frame b is triangulated through rig b % S in ONE launch
        (egotap_stereo_triangulate_streams).  The rigs live in a device table uploaded once; a captured graph holds the table's address and S, not the
        rigs, so ``update_stereo_rig`` needs no recapture.  The later of ``set_stereo_rig`` and ``set_stereo_rigs`` wins."""
        rigs = [self._parsed_rig("set_stereo_rigs", r) for r in rigs]
        if not 1 <= len(rigs) <= _spec.STEREO_MAX_STREAMS:
            raise ValueError(f"set_stereo_rigs: 1 .. {_spec.STEREO_MAX_STREAMS} rigs, one per stream, got {len(rigs)}")
        self._stereo_rigs = StreamRigs(rigs, min_score, self.net_AutoEncoder.preset.hm_size)
        self._stereo_rig = None

    def update_stereo_rig(self, s, left, right, t, R=None):
        """Stream ``s``'s rig replaced (a headset that joined or was recalibrated): checked, then written into row s of the device table(s) of
        ``set_stereo_rigs`` in place, ordered on the current stream.  Requests, graph replays and fusions enqueued afterwards serve the new rig;
        nothing is recaptured."""
        rigs = self.__dict__.get("_stereo_rigs")
        if rigs is None:
            raise _lib.EgotapError("update_stereo_rig: no per-stream rigs are set; call set_stereo_rigs(rigs) first")
        rigs.update(s, self._parsed_rig("update_stereo_rig", (left, right, t, R)))

    def _triangulation(self, who, wanted, affine=None, dev=None, B=0):
        """None, or what a serving entry needs for ``return_triangulation``: (the launch's host arguments, the capture key's part, the keypoint ->
        calibration pixel affines, pose_row0).  ``affine`` None: the RGB / byte entries' size / (4S) (``spec.stereo_pixel_affine``)."""
        if not wanted:
            return None
        rigs = self.__dict__.get("_stereo_rigs")
        if rigs is not None:      # a rig per stream: the launch reads the device table, and the capture key holds its address and S, not its contents
            if B % rigs.S:
                raise ValueError(f"{who}(return_triangulation=True): the batch must be a multiple of the {rigs.S} streams of set_stereo_rigs "
                                 f"(frame b uses rig b % S), got B = {B}")
            table = rigs.table(affine, dev)
            return _StreamTri(table, rigs.S), ("triangulation_streams", table.data_ptr(), rigs.S), affine, _spec.stereo_pose_row0(self.net_AutoEncoder.preset)
        rig = self.__dict__.get("_stereo_rig")
        if rig is None:
            raise _lib.EgotapError(f"{who}(return_triangulation=True): no stereo rig is set; call set_stereo_rig(left, right, t) first")
        left, right, t, R, min_score = rig
        p = self.net_AutoEncoder.preset
        if affine is None:
            affine = (_spec.stereo_pixel_affine(left, p.hm_size), _spec.stereo_pixel_affine(right, p.hm_size))
        affine = tuple(tuple(float(v) for v in row) for row in affine)
        return _lib.stereo_triangulate_args(left, right, t, R, affine, min_score), ("triangulation", rig, affine), affine, _spec.stereo_pose_row0(p)

    @torch.no_grad()
    def predict_pose_from_rgb(self, left, right, return_heatmaps=False, graphed=False, return_keypoints=False, return_limbs=False, return_triangulation=False):
        """Serving entry: stereo RGB [B, 3, 4S, 4S] x 2 -> pose [B, J(+1), 3], or (pose, heatmaps [B, 6J, S, S]) with ``return_heatmaps``.
        Replaces set_input() + evaluate() (utils/evaluate.py:104-114 without the metrics; egotap_autoencoder_model.py:177-223) for a caller
        that has no ground truth: no set_input, no loader keys, no autograd.  ONE library call (egotap_predict_pose_rgb): both estimators in
        eval mode (folded running statistics) in pieces of min(B, opt.hm_chunk) frames, then the pose-only head -- the same kernels, in
        the same order, as evaluate() on an eval-mode model, hence the same bits.  The networks' ``.training`` flags and precision are
        neither read for routing nor changed (this entry IS the inference forward); frozen networks (freeze_weights) are read from their
        arenas.  Without ``return_heatmaps`` in "bf16" precision at sides 64 / 128 the fp32 heatmaps are never written: conv_heatmap hands
        the head its bf16 operand directly (same pose bits; ``rgb_form()`` tells).

        ``return_keypoints``: also the 2D joints and confidences, float32 [B, 2, J, 4] (eye, joint, (x, y, score, index)) -- the peaks of the 2J
        position heatmaps (``lib.heatmap_peaks``, ``spec.heatmap_peaks_ref``) in pixels of the 4S x 4S input frame, appended to the result:
        (pose, keypoints) or (pose, heatmaps, keypoints).  One more launch inside the same library call (egotap_predict_pose_rgb_kp), reading the
        heatmaps in whichever form the call holds them, so the bf16 hand-off stays on; the pose bits do not change.

        ``return_limbs``: also each limb's elevation angle and 2D segment per eye, float32 [B, 2, J, 8] (eye, limb, (theta, coherence, x, y, phi,
        length, peak, mass)) -- the 2J (cos, sin) pairs of the limb heatmaps decoded (``lib.limb_decode``, ``spec.limb_decode_ref``), (x, y), phi and
        length in the keypoints' units, appended after the keypoints.  One more launch inside the same library call (egotap_predict_pose_rgb_kpl)
        on the same tensor; the hand-off stays on, the other outputs keep their bits.

        ``return_triangulation``: also the stereo keypoints triangulated through the rig of ``set_stereo_rig`` (``lib.stereo_triangulate``,
        ``spec.stereo_triangulate_ref``): joints3d float32 [B, J, 8] = (X, Y, Z, gap, den, s, disagree, valid) in the left camera's frame and frame
        float32 [B, 8] = (t_hat xyz, n, rms / max disagree, rms / max gap), appended as the last two results.  t_hat places the pelvis-relative pose
        in the left camera's frame; disagree and gap tell per joint whether to believe it; neither needs ground truth.  One more launch on the same
        stream right after the library call, on the keypoints (computed inside when ``return_keypoints`` is off, then not returned) and the pose of
        this call; every other output keeps its bits and the workspace its size.  Raises by name without a rig.

        ``graphed``: the whole pipeline through a captured graph, one per (B, precision, frozen state, return_heatmaps, return_keypoints, return_limbs,
        and with ``return_triangulation`` the rig and the pixel affine), with
        static input and output buffers as ``net_AutoEncoder.predict_pose_graphed``: the returned tensors are the graph's own (valid until the
        next call with the same key).

        By name, not through the one call: resnet50 / resnet101 estimators (no one-call forward), estimators with different backbones and
        networks set to different precisions run the existing module forwards (``forward_into`` x 2, chunked) followed by
        ``net_AutoEncoder.predict_pose`` -- ungraphed (``graphed=True`` raises there), and only with eval-mode networks."""
        p = self.net_AutoEncoder.preset
        S0 = 4 * p.hm_size
        for t in (left, right):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise _lib.EgotapError("predict_pose_from_rgb runs on the GPU only (no CPU fallback); move the frames to cuda")
        B = left.shape[0]
        if tuple(left.shape) != (B, 3, S0, S0) or tuple(right.shape) != (B, 3, S0, S0):
            raise ValueError(f"expected left / right [B, 3, {S0}, {S0}], got {tuple(left.shape)} / {tuple(right.shape)}")
        lib = _lib.load()
        left, right = left.detach().float().contiguous(), right.detach().float().contiguous()
        src = _Source("predict_pose_from_rgb", left, right, B, lib.egotap_predict_pose_rgb_workspace_bytes,
                      (lib.egotap_predict_pose_rgb, lib.egotap_predict_pose_rgb_kp, lib.egotap_predict_pose_rgb_kpl), (B,))
        return self._serve(src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation)

    @staticmethod
    def _served(pose, hm, kp, lb=None, tr=None):
        """what a serving entry returns: the pose alone, or the pose followed by the heatmaps, keypoints and / or limb records that were asked for, and
        last the triangulation's two records (joints3d, frame)"""
        extra = tuple(t for t in (hm, kp, lb) + (tuple(tr) if tr is not None else ()) if t is not None)
        return (pose,) + extra if extra else pose

    def camera_table(self, dev):
        """the fp32 [3, 256] value table of predict_pose_from_camera on `dev` (spec.rgb_u8_table; opt.rgb_mean / opt.rgb_std override the ImageNet
        statistics): one small tensor the model owns, handed to every byte entry -- the library allocates nothing.  Cached per (device, mean, std):
        changing opt.rgb_mean / opt.rgb_std between calls builds a new table (and, its address being part of the capture key, a new graph)."""
        key = (dev, tuple(getattr(self.opt, "rgb_mean", None) or ()), tuple(getattr(self.opt, "rgb_std", None) or ()))
        hit = self.__dict__.get("_camera_table")
        if hit is None or hit[0] != key:
            hit = self._camera_table = (key, torch.from_numpy(_spec.rgb_u8_table(self.opt)).to(dev))
        return hit[1]

    def _serve(self, src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation):
        """One request of a serving entry, whichever ``src`` (``_Source``) it reads: through the one library call, or -- where one handle cannot express
        the three networks (``_rgb_one_call_refusal``) -- through the module forwards, by name and ungraphed."""
        tri = self._triangulation(src.who, return_triangulation, src.triangulation_affine, src.left.device, src.B)
        why = self._rgb_one_call_refusal()
        if why is None:
            return self._serve_one_call(src, return_heatmaps, return_keypoints, return_limbs, graphed, tri)
        if graphed:
            raise _lib.EgotapError(f"{src.who}(graphed=True): {why}; this configuration runs {src.module_route}, ungraphed")
        return self._serve_modules(src, why, return_heatmaps, return_keypoints, return_limbs, tri)

    def _serve_modules(self, src, why, return_heatmaps, return_keypoints, return_limbs, tri):
        """the module route: the source's float frames through ``forward_into`` x 2 (chunked) and ``net_AutoEncoder.predict_pose``, then the standalone
        operators for the extra outputs"""
        # the modules' inference forwards refuse train mode (theirs is then the differentiable path): say so before anything runs
        for name in self.model_names:
            if getattr(self, "net_" + name).training:
                raise _lib.EgotapError(f"predict_pose_from_rgb: {why}; this configuration runs the module forwards, which need net_{name} in "
                                       "eval mode (model.eval())")
        p, B = self.net_AutoEncoder.preset, src.B
        left, right = src.float_frames() if src.float_frames else (src.left, src.right)
        dev = left.device
        chunk = max(1, min(B, int(getattr(self.opt, "hm_chunk", 256))))
        cat = torch.empty((B, p.in_channels, p.hm_size, p.hm_size), dtype=torch.float32, device=dev)
        J = p.n_joints_hm
        same = self.net_HeatMap.blocks == self.net_RotHeatMap.blocks          # one scratch for both estimators where their sizes agree
        for net, c0 in ((self.net_HeatMap, 0), (self.net_RotHeatMap, 2 * J)):
            ws = None if net.bottleneck else (self.net_HeatMap if same else net)._workspace(chunk, dev)
            for lo in range(0, B, chunk):
                net.forward_into(left[lo:lo + chunk], right[lo:lo + chunk], cat[lo:lo + chunk], c0, workspace=ws)
        pose = self.net_AutoEncoder.predict_pose(cat)
        kp = lb = None
        affine = src.keypoint_affine or [(4.0, 0.0, 4.0, 0.0)] * 2
        if return_keypoints or tri is not None:
            kp = _lib.heatmap_peaks(cat, 0, 2 * J, groups=2, affine=affine).view(B, 2, J, 4)
        if return_limbs:
            lb = _lib.limb_decode(cat, 2 * J, J, eyes=2, affine=affine)
        tr = None
        if tri is not None and isinstance(tri[0], _StreamTri):
            tr = _lib.stereo_triangulate_streams(kp, tri[0].table, tri[0].S, pose=pose, pose_row0=tri[3])
        elif tri is not None:
            rig_l, rig_r, rig_t, rig_R, min_score = self._stereo_rig
            tr = _lib.stereo_triangulate(kp, rig_l, rig_r, rig_t, R=rig_R, affine=tri[2], min_score=min_score, pose=pose, pose_row0=tri[3])
        return self._served(pose, cat if return_heatmaps else None, kp if return_keypoints else None, lb, tr)

    @staticmethod
    def _launch(src, h, left, right, out, chunk, ws, dev, tri):
        """the source's ABI entry on ``out`` = (pose, heatmaps, keypoints, limbs, triangulation records), picked by the outputs present -- limbs: _kpl; no
        keypoints: the base entry; otherwise _kp -- and, with ``tri``, the triangulation launch behind it on the same stream"""
        pose, hm, kp, lb, tr = out
        fn, extra = (src.entries[2], (ptr(kp), ptr(lb))) if lb is not None else (src.entries[0], ()) if kp is None else (src.entries[1], (ptr(kp),))
        _lib.check(fn(h, ptr(left), ptr(right), *src.args, ptr(pose), ptr(hm), chunk, ptr(ws), ws.numel(), stream(dev), *extra))
        if tri is not None and isinstance(tri[0], _StreamTri):
            _lib.stereo_triangulate_streams_into(tri[0].table, tri[0].S, kp, pose, tri[3], tr[0], tr[1], dev)
        elif tri is not None:
            _lib.stereo_triangulate_into(tri[0], kp, pose, tri[3], tr[0], tr[1], dev)

    def _serve_one_call(self, src, return_heatmaps, return_keypoints, return_limbs, graphed, tri):
        """The host side of a one-call serving entry on the serving handle: outputs, workspace (eager: the handle's grow-only one; graphed: the
        graph's own), capture and replay with static inputs of the frames' dtype.  ``src.size_query(h, B, chunk, &bytes)`` and ``_launch`` are the
        entry's two ABI calls; ``src.kind`` extends the capture key, ``src.keep`` is what a graph must keep alive besides its own buffers.  ``tri``
        (``_triangulation``): the triangulation launch follows the library call on the same stream -- inside a capture too, so a graphed request stays
        one replay -- on keypoints that exist for it alone when they were not asked for."""
        p, B, left, right = self.net_AutoEncoder.preset, src.B, src.left, src.right
        dev = left.device
        chunk = max(1, min(B, int(getattr(self.opt, "hm_chunk", 256))))

        def f32(*shape):
            return torch.empty((B,) + shape, dtype=torch.float32, device=dev)
        out = (f32(p.out_joints, 3),
               f32(p.in_channels, p.hm_size, p.hm_size) if return_heatmaps else None,
               f32(2, p.n_joints_hm, 4) if return_keypoints or tri is not None else None,
               f32(2, p.n_joints_hm, 8) if return_limbs else None,
               (f32(p.n_joints_hm, 8), f32(8)) if tri is not None else None)

        def served(out):
            pose, hm, kp, lb, tr = out
            return self._served(pose, hm, kp if return_keypoints else None, lb, tr)
        if B == 0:
            return served(out)
        with torch.cuda.device(dev):
            st = self._rgb_state(dev)
            self._rgb_attach_act_scratch(st, B, dev)
            h = st.handle.h
            need = _session.nbytes(src.size_query, h, B, chunk)
            if not graphed:
                _session.grown(st, "ws", need, dev, drop_first=True)
                st.chunk = chunk
                self._launch(src, h, left, right, out, chunk, st.ws, dev, tri)
                return served(out)
            # one graph per (batch, heatmaps wanted, keypoints wanted, limbs wanted, precision, frozen arenas, bound tensors, chunk, source): every pointer a captured
            # launch takes is baked in, so the graph owns its buffers -- static inputs and outputs, a workspace of its own -- and keeps the scratch
            # buffers and arenas alive
            nets = (self.net_AutoEncoder, self.net_HeatMap, self.net_RotHeatMap)
            key = (B, bool(return_heatmaps), bool(return_keypoints), bool(return_limbs), st.precision, tuple(st.frozen),
                   tuple(st.handle.bound[i] for i in (_lib.NET_LIFT, _lib.NET_HM_POS, _lib.NET_HM_ROT)), chunk, str(dev)) + tuple(src.kind)
            if tri is not None:
                key += (tri[1],)

            def build():
                s_l, s_r = left.clone(), right.clone()
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                held = (ws, st.wscratch, st.ascratch) + tuple(src.keep) + tuple(n._frozen_arena for n in nets if n.weights_frozen)
                if tri is not None and isinstance(tri[0], _StreamTri):
                    held += (tri[0].table,)
                return (lambda: self._launch(src, h, s_l, s_r, out, chunk, ws, dev, tri)), (s_l, s_r, out), held
            graph, (s_l, s_r, out), _ = _session.captured(st.graphs, key, build)
            s_l.copy_(left)
            s_r.copy_(right)
            graph.replay()
        return served(out)

    @torch.no_grad()
    def predict_pose_from_camera(self, left8, right8, return_heatmaps=False, graphed=False, return_keypoints=False, return_limbs=False, return_triangulation=False):
        """predict_pose_from_rgb from what a camera delivers: stereo frames uint8 [B, 4S, 4S, 3] (HWC, RGB order, already at 4S x 4S) -> pose
        [B, J(+1), 3], or (pose, heatmaps) with ``return_heatmaps``.  ONE library call (egotap_predict_pose_rgb_u8) on the serving handle of
        predict_pose_from_rgb: the caller's astype(float32) / 255, normalisation, HWC -> CHW and the four-fold upload are gone -- at sides 64 / 128
        the stem kernels look every byte up in a 768-entry table (``camera_table``) while they stage it; at other sides the library converts chunk
        by chunk into a workspace slice.  The bits are those of predict_pose_from_rgb on the gathered frames table[c][byte].  ``return_keypoints``: as
        predict_pose_from_rgb, in pixels of the 4S x 4S frame (egotap_predict_pose_rgb_u8_kp).  ``return_limbs``: as predict_pose_from_rgb
        (egotap_predict_pose_rgb_u8_kpl).  ``return_triangulation``: as predict_pose_from_rgb.

        ``graphed``: as predict_pose_from_rgb, with static BYTE inputs; the capture key also holds the source kind and the table, so the two entries
        never share a graph.  Configurations one handle cannot express (Bottleneck backbones, mixed backbones or precisions) run
        egotap_rgb_u8_to_f32 followed by predict_pose_from_rgb's module route -- by name, ungraphed."""
        S0 = 4 * self.net_AutoEncoder.preset.hm_size
        B = _lib.check_camera_frames("predict_pose_from_camera", left8, right8, S0)
        lib, table = _lib.load(), self.camera_table(left8.device)
        src = _Source("predict_pose_from_camera", left8, right8, B, lib.egotap_predict_pose_rgb_u8_workspace_bytes,
                      (lib.egotap_predict_pose_rgb_u8, lib.egotap_predict_pose_rgb_u8_kp, lib.egotap_predict_pose_rgb_u8_kpl), (B, ptr(table)),
                      kind=("u8", table.data_ptr()), keep=(table,), float_frames=lambda: _lib.rgb_u8_to_f32(left8, right8, table),
                      module_route="the converter and the module forwards")
        return self._serve(src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation)

    @torch.no_grad()
    def predict_pose_from_sensor(self, left8, right8, crop=None, crop_right=None, mirror_right=False, return_heatmaps=False, graphed=False,
                                 return_keypoints=False, return_limbs=False, return_triangulation=False):
        """predict_pose_from_camera from the sensor's own frames: stereo uint8 [B, H, W, 3] (HWC, RGB, any H x W, the same for both eyes) -> pose
        [B, J(+1), 3], or (pose, heatmaps) with ``return_heatmaps``.  ONE library call (egotap_predict_pose_sensor_u8) on the serving handle:
        the caller's crop, flip, F.interpolate and round to bytes are gone -- the library resizes chunk by chunk into a workspace slice
        (rgb_u8_resize_kernel) and the byte source reads that slice.  The bits are those of predict_pose_from_camera on
        ``spec.resize_u8(frames, rect, mirror, 4S)``, the integer restatement of the resize (within 0.5 + 510 / 4096 of exact bilinear
        interpolation with align_corners=False on every byte).

        ``crop``: the source rectangle (x0, y0, w, h) in source pixels, inside the frame (None: the full frame); ``crop_right``: the right eye's
        (None: the same as ``crop``).  ``mirror_right``: the right eye's output column X takes what column 4S - 1 - X takes without it.  The
        reference flips the second camera's frame and THEN crops (reprocess_egocap_data.py:100-104, :221): its rectangle x0' in flipped
        coordinates is x0 = W - x0' - w here.  Frames already 4S x 4S with the full rectangle and no mirror are read in place.

        ``return_keypoints``: as predict_pose_from_rgb, but in pixels of each eye's SENSOR frame (egotap_predict_pose_sensor_u8_kp): the inverse of the
        resize's map, per eye from its own rectangle and mirror flag (``spec.sensor_keypoint_affine``).  ``return_limbs``: as predict_pose_from_rgb,
        (x, y), phi and length in the same sensor pixels (egotap_predict_pose_sensor_u8_kpl); a rectangle whose w / S and h / S differ bends phi
        and length (the blur is no longer isotropic in the output frame).  ``return_triangulation``: as predict_pose_from_rgb, with the identity as the
        pixel affine: the calibration is the sensor's, and the keypoints are already in sensor pixels with crop and mirror undone.

        ``graphed``: as predict_pose_from_camera; the capture key holds the source kind, H, W, the rectangles, the mirror flags and the table, so
        no graph is shared with the other entries.  Configurations one handle cannot express (Bottleneck backbones, mixed backbones or precisions)
        run egotap_rgb_u8_resize followed by predict_pose_from_camera's fallback -- by name, ungraphed."""
        p = self.net_AutoEncoder.preset
        S0 = 4 * p.hm_size
        B, H, W = _lib.check_sensor_frames("predict_pose_from_sensor", left8, right8)
        rect_l = _spec.check_resize_rect("predict_pose_from_sensor", crop, H, W)
        rect_r = _spec.check_resize_rect("predict_pose_from_sensor", crop if crop_right is None else crop_right, H, W)
        mirrors = (0, int(bool(mirror_right)))
        lib, table = _lib.load(), self.camera_table(left8.device)

        def float_frames():
            return _lib.rgb_u8_to_f32(*_lib.rgb_u8_resize(left8, right8, S0, rect_l, rect_r, False, bool(mirror_right)), table)
        src = _Source("predict_pose_from_sensor", left8, right8, B,
                      lambda h, b, chunk, out: lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, b, H, W, chunk, out),
                      (lib.egotap_predict_pose_sensor_u8, lib.egotap_predict_pose_sensor_u8_kp, lib.egotap_predict_pose_sensor_u8_kpl),
                      (B, H, W, (C.c_int * 8)(*rect_l, *rect_r), (C.c_int * 2)(*mirrors), ptr(table)),
                      kind=("sensor", H, W, rect_l + rect_r, mirrors, table.data_ptr()), keep=(table,), float_frames=float_frames,
                      keypoint_affine=[_spec.sensor_keypoint_affine(rect_l, False, p.hm_size), _spec.sensor_keypoint_affine(rect_r, bool(mirror_right), p.hm_size)],
                      triangulation_affine=_spec.STEREO_IDENTITY_AFFINE, module_route="the resize, the converter and the module forwards")
        return self._serve(src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation)

    @torch.no_grad()
    def predict_pose_from_sensor_yuv(self, left8, right8, layout, colour=_spec.YuvColour("bt601", "limited"), crop=None, crop_right=None, mirror_right=False,
                                     return_heatmaps=False, graphed=False, return_keypoints=False, return_limbs=False, return_triangulation=False):
        """predict_pose_from_sensor from the camera's own buffer: stereo NV12 or YUYV frames, uint8, B frames of ``layout.frame_stride`` bytes per eye
        (``spec.YuvLayout``: format, H, W, row pitch, chroma offset; ``lib.check_yuv_frames``) -> pose [B, J(+1), 3].  ONE library call
        (egotap_predict_pose_sensor_yuv) on the serving handle: the caller's plane unpacking, float colour conversion, rounding and the three-bytes-per-pixel
        upload are gone -- the library converts and resizes chunk by chunk into the sensor entry's workspace slice (yuv_u8_resize_kernel) and the byte
        source reads that slice.  The bits are those of predict_pose_from_sensor on ``spec.yuv_to_rgb_u8(frames, layout, colour)``, the integer
        restatement of the conversion (``spec.YuvColour``: matrix bt601 / bt709, range limited / full; chroma replicated, nothing interpolated in YUV).
        A YUV source always converts: there is no in-place identity request.

        ``crop``, ``crop_right``, ``mirror_right``, ``return_keypoints``, ``return_limbs``, ``return_triangulation``: as predict_pose_from_sensor, in
        pixels of the H x W sensor frame.  ``graphed``: as predict_pose_from_sensor; the capture key holds the source kind, the layout, the colour, the
        rectangles, the mirror flags and the table, so no graph is shared with the other entries.  Configurations one handle cannot express (Bottleneck
        backbones, mixed backbones or precisions) run egotap_yuv_u8_resize followed by predict_pose_from_camera's fallback -- by name, ungraphed."""
        p = self.net_AutoEncoder.preset
        S0 = 4 * p.hm_size
        who = "predict_pose_from_sensor_yuv"
        if not isinstance(layout, _spec.YuvLayout) or not isinstance(colour, _spec.YuvColour):
            raise ValueError(f"{who}: layout is a spec.YuvLayout and colour a spec.YuvColour, got {type(layout).__name__} / {type(colour).__name__}")
        B = _lib.check_yuv_frames(who, left8, right8, layout)
        H, W = layout.H, layout.W
        rect_l = _spec.check_resize_rect(who, crop, H, W)
        rect_r = _spec.check_resize_rect(who, crop if crop_right is None else crop_right, H, W)
        mirrors = (0, int(bool(mirror_right)))
        lib, table = _lib.load(), self.camera_table(left8.device)
        desc = _lib.yuv_source(layout, colour)

        def float_frames():
            return _lib.rgb_u8_to_f32(*_lib.yuv_u8_resize(left8, right8, layout, colour, S0, rect_l, rect_r, False, bool(mirror_right)), table)
        src = _Source(who, left8, right8, B,
                      lambda h, b, chunk, out: lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, b, H, W, chunk, out),
                      (lib.egotap_predict_pose_sensor_yuv, lib.egotap_predict_pose_sensor_yuv_kp, lib.egotap_predict_pose_sensor_yuv_kpl),
                      (B, C.byref(desc), (C.c_int * 8)(*rect_l, *rect_r), (C.c_int * 2)(*mirrors), ptr(table)),
                      kind=("sensor_yuv", layout, colour, rect_l + rect_r, mirrors, table.data_ptr()), keep=(table,), float_frames=float_frames,
                      keypoint_affine=[_spec.sensor_keypoint_affine(rect_l, False, p.hm_size), _spec.sensor_keypoint_affine(rect_r, bool(mirror_right), p.hm_size)],
                      triangulation_affine=_spec.STEREO_IDENTITY_AFFINE, module_route="the conversion and resize, the converter and the module forwards")
        return self._serve(src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation)

    def lens_maps(self, left, right=None, fill=(0, 0, 0), device=None):
        """The rig's two lens maps for ``predict_pose_from_lens``: ``left`` / ``right`` a ``spec.LensMap`` each (``spec.lens_map(model_camera,
        sensor, 4 * hm_size, R, frame_size, mirror)``), uploaded ONCE to ``device`` (None: the current GPU); returns the handle object that keeps the
        device tensors (``lib.LensMaps``).  Refused by name: maps whose S0 is not 4 * hm_size, and maps that differ between the eyes in S0, the
        sensor frame's (H, W) or the model camera's calibration size (one descriptor serves both eyes).  ``fill``: the (R, G, B) of a pixel the
        sensor does not see, for both eyes or one triple per eye.  A rig per stream: ``left`` a list of per-stream (left_map, right_map) pairs and
        ``right`` None; the result has ``.S`` streams and ``predict_pose_from_lens`` gathers frame b of a time-major batch through pair b % S."""
        S0 = 4 * self.net_AutoEncoder.preset.hm_size
        pairs = left if right is None and isinstance(left, (list, tuple)) else ()
        for m in (left, right) + tuple(m for pair in pairs if isinstance(pair, (list, tuple)) for m in pair):
            if isinstance(m, _spec.LensMap) and m.S0 != S0:
                raise ValueError(f"lens_maps: the estimators read {S0} x {S0} frames (4 * hm_size), the map was built for S0 = {m.S0}")
        return _lib.lens_maps(left, right, fill, device)

    @torch.no_grad()
    def predict_pose_from_lens(self, left8, right8, maps, layout=None, colour=_spec.YuvColour("bt601", "limited"), return_heatmaps=False, graphed=False,
                               return_keypoints=False, return_limbs=False, return_triangulation=False):
        """predict_pose_from_sensor for a rig whose lens is not the one the estimators were trained on: stereo frames of the sensor's own H x W ->
        pose [B, J(+1), 3].  ``maps`` (``lens_maps``) says per eye where in the sensor's frame each pixel of the model camera's 4S x 4S frame is
        sampled; ``layout`` None: uint8 [B, H, W, 3] frames, a ``spec.YuvLayout``: the camera's NV12 / YUYV buffer with its ``colour``.  ONE library
        call (egotap_predict_pose_lens) on the serving handle: the caller's cv2.remap on the host and the three-bytes-per-pixel upload are gone -- the
        library gathers chunk by chunk into the sensor entry's workspace slice (lens_remap_kernel) and the byte source reads that slice.  The bits are
        those of predict_pose_from_camera on ``spec.lens_remap_u8(frames, map, fill)`` (for YUV: of the frames ``spec.yuv_to_rgb_u8`` gives), the
        integer restatement of the gather.  A lens source always gathers: there is no in-place identity request.

        ``return_keypoints`` / ``return_limbs``: as predict_pose_from_sensor, in pixels of the MODEL camera's calibration image
        (egotap_predict_pose_lens_kp / _kpl): per eye ``spec.sensor_keypoint_affine((0, 0, model_w, model_h), mirror, S)``;
        ``spec.lens_map_points`` takes them on to the sensor's frame for drawing.  ``return_triangulation``: as predict_pose_from_sensor, with the
        identity as the pixel affine -- the rig of ``set_stereo_rig`` is then the two MODEL cameras, with the R and t of the virtual rig the maps
        render.  ``graphed``: as predict_pose_from_sensor; the capture key holds the source kind, the format, the layout, the colour, both map addresses,
        the fill and the table.  Configurations one handle cannot express (Bottleneck backbones, mixed backbones or precisions) run egotap_lens_remap
        followed by predict_pose_from_camera's fallback -- by name, ungraphed."""
        p = self.net_AutoEncoder.preset
        S0 = 4 * p.hm_size
        who = "predict_pose_from_lens"
        B = _lib.check_lens_frames(who, left8, right8, maps, layout, colour)
        if maps.S0 != S0:
            raise ValueError(f"{who}: the estimators read {S0} x {S0} frames (4 * hm_size), the maps were built for S0 = {maps.S0}")
        per_stream = maps.S > 1      # a map per stream: the _streams entries, frame b through map b % S
        if B % maps.S:
            raise ValueError(f"{who}: the batch must be a multiple of the maps' {maps.S} streams (frame b uses map b % S), got B = {B}")
        lib, table = _lib.load(), self.camera_table(left8.device)
        desc = _lib.lens_source(maps, layout, colour)
        model_h, model_w = maps.model_size

        def float_frames():
            return _lib.rgb_u8_to_f32(*(_lib.lens_remap_streams if per_stream else _lib.lens_remap)(left8, right8, maps, S0, layout, colour), table)
        entries = (lib.egotap_predict_pose_lens, lib.egotap_predict_pose_lens_kp, lib.egotap_predict_pose_lens_kpl)
        if per_stream:
            entries = (lib.egotap_predict_pose_lens_streams, lib.egotap_predict_pose_lens_streams_kp, lib.egotap_predict_pose_lens_streams_kpl)
        src = _Source(who, left8, right8, B, lib.egotap_predict_pose_lens_workspace_bytes, entries,
                      (B, C.byref(desc), maps.S, ptr(table)) if per_stream else (B, C.byref(desc), ptr(table)),
                      kind=(("lens_streams", maps.S) if per_stream else ("lens",)) + ("rgb8" if layout is None else layout.format, layout,
                                                                                      colour if layout is not None else None) + maps.key
                      + (maps.H, maps.W, maps.model_size, maps.mirrors, table.data_ptr()),
                      keep=(table, maps, desc), float_frames=float_frames,
                      keypoint_affine=[_spec.sensor_keypoint_affine((0, 0, model_w, model_h), bool(m), p.hm_size) for m in maps.mirrors],
                      triangulation_affine=_spec.STEREO_IDENTITY_AFFINE, module_route="the lens remap, the converter and the module forwards")
        return self._serve(src, return_heatmaps, graphed, return_keypoints, return_limbs, return_triangulation)

    def new_pose_tracker(self, streams=1, params=None, world=False, ortho_tol=None):
        """A ``PoseTracker`` for this model's outputs: P = the lifted pose's rows, J = the heatmap joints the triangulation returns; ``streams`` camera
        rigs side by side, ``params`` a ``spec.TrackParams`` (None: its defaults, which nobody has tuned on real data).  Feed it what a serving entry
        returns: ``pose, joints3d, frame = model.predict_pose_from_camera(l8, r8, return_triangulation=True)``;
        ``placed, tracks = tracker.update(pose, joints3d, frame, dt=1 / 30)``.  The serving entries, their graphs and their outputs do not change.
        ``world=True``: the tracker follows the skeleton in a world frame from the headset's own pose,
        ``placed_world, tracks, placed_cam = tracker.update(pose, joints3d, frame, dt=1 / 30, rig_pose=spec.rig_pose(t, quat=q) on the device)``;
        ``ortho_tol`` (None: 1e-6; a world tracker's alone) bounds how far a rig pose's matrix may be from a rotation and still count."""
        p = self.net_AutoEncoder.preset
        return PoseTracker(p.out_joints, p.n_joints_hm, streams=streams, params=params, world=world, ortho_tol=ortho_tol)

    def new_stereo_fusion(self, sigma_prior, params=None, affine=None):
        """A ``StereoFusion`` for this model's outputs and the rig of ``set_stereo_rig``:
        ``pose, kp, joints3d, frame = model.predict_pose_from_camera(l8, r8, return_keypoints=True, return_triangulation=True)``;
        ``pose_fused, fused, stats = fusion.update(pose, kp, frame)``; ``placed, tracks = tracker.update(pose_fused, joints3d, frame, dt=1 / 30)``.
        ``sigma_prior``: the standard deviation of a lifted joint in the pose's units -- required, the project knows no dataset's; ``params`` a
        ``spec.FuseParams`` for the other fields (None: its defaults, which nobody has tuned on real data; its sigma_prior must then agree).
        ``affine``: None for the RGB / byte entries' keypoints (``spec.stereo_pixel_affine``), ``"identity"`` for the sensor and lens entries', or an
        explicit [2, 4].  The serving entries, the trackers, their graphs and their outputs do not change."""
        rigs = self.__dict__.get("_stereo_rigs")
        rig = self.__dict__.get("_stereo_rig")
        if rig is None and rigs is None:
            raise _lib.EgotapError("new_stereo_fusion: no stereo rig is set; call set_stereo_rig(left, right, t) first")
        if params is None:
            params = _spec.FuseParams(sigma_prior=sigma_prior)
        elif not isinstance(params, _spec.FuseParams) or params.sigma_prior != float(sigma_prior):
            raise ValueError(f"new_stereo_fusion: params is a spec.FuseParams whose sigma_prior is the one given ({sigma_prior}), got {params!r}")
        p = self.net_AutoEncoder.preset
        if isinstance(affine, str):
            if affine != "identity":
                raise ValueError(f'new_stereo_fusion: affine is None, "identity" or a [2, 4] of (ax, bx, ay, by) per eye, got {affine!r}')
            affine = _spec.STEREO_IDENTITY_AFFINE
        if rigs is not None:      # a rig per stream: the fusion reads the model's table (None: each stream's own pixel affine), so update_stereo_rig is seen
            return StreamStereoFusion(rigs, params, affine=affine, pose_row0=_spec.stereo_pose_row0(p))
        left, right, t, R, min_score = rig
        if affine is None:
            affine = (_spec.stereo_pixel_affine(left, p.hm_size), _spec.stereo_pixel_affine(right, p.hm_size))
        return StereoFusion(left, right, t, params, R=R, affine=affine, min_score=min_score, pose_row0=_spec.stereo_pose_row0(p))

    def new_skeleton(self, rig=None, streams=1, params=None, twist=None):
        """A ``Skeleton`` for this model's pose rows: rigid bones and a rotation per bone from what a tracker returns,
        ``placed, tracks = tracker.update(...)``; ``rigid, rotations, lengths = skeleton.update(placed, tracks)`` -- one more launch on the same stream.
        ``rig`` a ``spec.skeleton_rig(...)`` of the avatar (its rest pose, and its own bone lengths to retarget); None: the skeleton refuses to update
        until ``set_rest_pose(pose_rows)`` has taken one frame as the rest pose -- the project ships no avatar.  ``params`` a ``spec.SkeletonParams``
        (None: its defaults, which nobody has tuned on real data).  ``twist`` a ``spec.skeleton_twist(rig, ...)`` of that rig: bones with a pole then
        also roll about their own axis (None: they follow their parent, until ``set_hinges(pose_rows)`` has taken a frame with bent elbows and knees).
        The serving entries, the trackers, their graphs and their outputs do not change."""
        return Skeleton(self.net_AutoEncoder.preset.out_joints, joint_preset=self.opt.joint_preset, rig=rig, streams=streams, params=params, twist=twist)

    def new_overlay(self, style=None):
        """An ``Overlay`` for this model's outputs: ``pose, hm, kp = model.predict_pose_from_camera(l8, r8, return_heatmaps=True, return_keypoints=True)``;
        ``out_l, out_r = ov.draw(l8, r8, keypoints=kp, heatmaps=hm)`` -- the frames with the position heatmaps, the skeleton's bones and the keypoints
        drawn on, one or two launches behind the serving call on the same stream.  ``style`` a ``spec.OverlayStyle`` with one mark per heatmap joint
        (None: ``spec.overlay_style(joint_preset)``, which nobody has tuned).  The serving entries, their graphs and their outputs do not change."""
        return Overlay(self.net_AutoEncoder.preset.n_joints_hm, _spec.overlay_style(self.opt.joint_preset) if style is None else style)

    def rgb_intermediate(self, name: str, B: int):
        """View of the heatmaps the last UNGRAPHED predict_pose_from_rgb(return_heatmaps=False) call of batch B kept inside its workspace (parity
        tests; egotap_debug.h): "heatmaps" -> fp32 [B, 6J, S, S] after a "scratch" call, "handoff" -> bfloat16 [B, 6J, S, S] after a "handoff" call"""
        st, p = self.__dict__.get("_rgb"), self.net_AutoEncoder.preset
        if st is None or st.ws is None or st.chunk is None:
            raise _lib.EgotapError("rgb_intermediate: no ungraphed one-call predict_pose_from_rgb has run on this model yet (a graph keeps its own workspace)")
        view = st.handle.intermediate(_lib.load().egotap_debug_predict_pose_rgb_intermediate, st.ws, B, st.chunk, name=name,
                                      dtype=torch.bfloat16 if name == "handoff" else torch.float32)
        return view.view(B, p.in_channels, p.hm_size, p.hm_size)

    # ---- checkpoints (base_model.py:64-148 file naming) --------------------------------------------------------
    def save_networks(self, which_epoch=None, checkpoint_path=None):
        if which_epoch is None and checkpoint_path is None:
            raise ValueError("which_epoch and checkpoint_path cannot be both None")
        which_epoch = "checkpoint" if which_epoch is None else which_epoch
        checkpoint_path = self.save_dir if checkpoint_path is None else checkpoint_path
        os.makedirs(checkpoint_path, exist_ok=True)
        for name in self.model_names:
            net = getattr(self, "net_" + name)
            sd = OrderedDict((k, v.detach().cpu()) for k, v in net.state_dict().items())
            torch.save(sd, os.path.join(checkpoint_path, "%s_net_%s.pth" % (which_epoch, name)))
        for i, o in enumerate(self.optimizers):                      # base_model.py:83-92
            torch.save(o.state_dict(), os.path.join(checkpoint_path, "%s_optim_%s.pth" % (which_epoch, i)))
        for i, sch in enumerate(self.schedulers):
            torch.save(sch.state_dict(), os.path.join(checkpoint_path, "%s_scheduler_%s.pth" % (which_epoch, i)))
        if isinstance(which_epoch, int) and which_epoch > 1 and which_epoch != getattr(self.opt, "epoch_count", None):
            prev = which_epoch - 1                                   # base_model.py:94-114: keep only the latest numbered epoch
            names = ["%s_net_%s.pth" % (prev, n) for n in self.model_names]
            names += ["%s_optim_%s.pth" % (prev, i) for i in range(len(self.optimizers))]
            names += ["%s_scheduler_%s.pth" % (prev, i) for i in range(len(self.schedulers))]
            for fn in names:
                fp = os.path.join(checkpoint_path, fn)
                if os.path.exists(fp):
                    os.remove(fp)

    def load_optimizers(self, which_epoch="checkpoint", checkpoint_path=None):
        """resume: optimizer / scheduler state written by save_networks (also accepts torch.optim.AdamW state files)"""
        checkpoint_path = self.save_dir if checkpoint_path is None else checkpoint_path
        for i, o in enumerate(self.optimizers):
            o.load_state_dict(torch.load(os.path.join(checkpoint_path, "%s_optim_%s.pth" % (which_epoch, i)), map_location=self.device))
        for i, sch in enumerate(self.schedulers):
            sch.load_state_dict(torch.load(os.path.join(checkpoint_path, "%s_scheduler_%s.pth" % (which_epoch, i))))

    def load_networks(self, which_epoch=None, net=None, path_to_trained_weights=None, checkpoint_path=None):
        if path_to_trained_weights is not None:
            # base_model.py:136-146: "./log/" is stripped and the rest joined with opt.log_dir; module. prefixes of a
            # DataParallel checkpoint are dropped under --distributed (here: always, it is harmless)
            if "./log" in path_to_trained_weights:
                path_to_trained_weights = path_to_trained_weights.replace("./log/", "")
            weight_path = os.path.join(getattr(self.opt, "log_dir", "./log"), path_to_trained_weights)
            sd = torch.load(weight_path, map_location="cpu")
            sd = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in sd.items())
            net.load_state_dict(sd)
            return
        if which_epoch is None and checkpoint_path is None:
            raise ValueError("which_epoch and checkpoint_path cannot be both None")
        which_epoch = "checkpoint" if which_epoch is None else which_epoch
        checkpoint_path = self.save_dir if checkpoint_path is None else checkpoint_path
        for name in self.model_names:
            n = getattr(self, "net_" + name)
            n.load_state_dict(torch.load(os.path.join(checkpoint_path, "%s_net_%s.pth" % (which_epoch, name)), map_location="cpu"))
            n.eval() if not self.isTrain else n.train()

    def get_current_errors(self):
        return OrderedDict((n, getattr(self, "loss_" + n).item()) for n in self.loss_names if hasattr(self, "loss_" + n))

    def update_learning_rate(self):
        for s in self.schedulers:
            s.step()


class HeatmapSharedModel(nn.Module):
    """Stage-1 wrapper: trains / evaluates one heatmap estimator (reference: model/heatmap_shared_model.py).  Same surface as the
    reference (set_input keys, forward, optimize_parameters, evaluate -> mse_heatmap, loss_* attributes, save / load); the network,
    the losses and the optimizer step run on HIP kernels (egotap_amd/hm_training.py), PyTorch is autograd glue only.
    Built for the two shipped configurations: the position net (num_rot_heatmap = 0) or the sin/cos limb net (num_heatmap = 0)."""

    def name(self):
        return "Heatmap Shared model"

    def initialize(self, opt):
        self.opt = opt
        self.gpu_ids = getattr(opt, "gpu_ids", [0])
        self.isTrain = getattr(opt, "isTrain", False)
        self.save_dir = os.path.join(getattr(opt, "log_dir", "./log"), getattr(opt, "experiment_name", "experiment"))
        self.device = torch.device("cuda:{}".format(self.gpu_ids[0])) if self.gpu_ids else torch.device("cuda:0")
        if not getattr(opt, "stereo", True):
            raise NotImplementedError("only the stereo presets are built")
        if opt.num_heatmap > 0 and opt.num_rot_heatmap > 0:
            raise NotImplementedError("train the position net and the limb net separately (the shipped stage-1 scripts do)")
        self.is_limb = opt.num_rot_heatmap > 0
        self.loss_names = ["limb_heatmap_left", "limb_heatmap_right"] if self.is_limb else ["heatmap_left", "heatmap_right"]
        self.model_names = ["HeatMap"]
        self.visual_names, self.visual_pose_names = ["input_rgb_left", "input_rgb_right"], []
        self.eval_key, self.cm2mm = "mse_heatmap", 10
        self.net_HeatMap = networks.HeatMap_UnrealEgo_Shared(opt, getattr(opt, "model_name", "resnet18"), 2)
        if self.isTrain and self.net_HeatMap.bottleneck:
            raise NotImplementedError(f"stage-1 training of a {self.net_HeatMap.model_name} estimator is not built (resnet18 / resnet34 are); "
                                      "its checkpoints load and run in evaluation and as frozen estimators of stage 2")
        self.optimizers, self.schedulers = [], []
        self.to(self.device)
        # --use_amp (heatmap_shared_model.py:17, 99, 111: fp16 autocast + GradScaler): the reduced-precision HIP mode of the
        # estimator's convolutions (split-bf16 matrix-core products, fp32 accumulate, fp32 master weights; no scaler needed)
        if self.isTrain and getattr(opt, "use_amp", False):
            self.net_HeatMap.set_precision(getattr(opt, "amp_precision_heatmap", "bf16x3"))
        if self.isTrain and getattr(opt, "path_to_trained_heatmap", None) is not None:
            self.load_networks(net=self.net_HeatMap, path_to_trained_weights=opt.path_to_trained_heatmap)   # heatmap_shared_model.py:60-64
        if self.isTrain:
            if getattr(opt, "weight_decay", 0.0) != 0.0:
                raise NotImplementedError("torch.optim.Adam's L2 weight decay is not built (the shipped scripts use 0)")
            from .training import EgotapAdamW, get_scheduler
            # torch.optim.Adam(lr, weight_decay=0) == AdamW with zero decay: same kernel (heatmap_shared_model.py:69-73, eps 1e-8)
            self.optimizer_HeatMap = EgotapAdamW(self.net_HeatMap.parameters(), lr=getattr(opt, "lr", 1e-3), eps=1e-8, weight_decay=0.0)
            self.optimizers.append(self.optimizer_HeatMap)
            if getattr(opt, "lr_policy", None):
                self.schedulers = [get_scheduler(o, opt) for o in self.optimizers]

    def set_input(self, data):
        self.data = data
        dev = self.device
        self.input_rgb_left = data["input_rgb_left"].to(dev).float().contiguous()
        self.input_rgb_right = data["input_rgb_right"].to(dev).float().contiguous()
        if self.is_limb:
            self.gt_limb_heatmap_left, self.gt_limb_heatmap_right = data["gt_limb_heatmap_left"].to(dev), data["gt_limb_heatmap_right"].to(dev)
            self.gt_plength_left, self.gt_plength_right = data["gt_plength_left"].to(dev), data["gt_plength_right"].to(dev)
            self._gt = torch.cat((self.gt_limb_heatmap_left, self.gt_limb_heatmap_right), 1).float().contiguous()
            self._plen = torch.cat((self.gt_plength_left, self.gt_plength_right), 1).float().contiguous()
        else:
            self.gt_heatmap_left, self.gt_heatmap_right = data["gt_heatmap_left"].to(dev), data["gt_heatmap_right"].to(dev)
            self._gt = torch.cat((self.gt_heatmap_left, self.gt_heatmap_right), 1).float().contiguous()
            self._plen = None

    def forward(self):
        self.pred_heatmap_cat = self.net_HeatMap(self.input_rgb_left, self.input_rgb_right)
        n = self.pred_heatmap_cat.shape[1] // 2
        left, right = self.pred_heatmap_cat[:, :n], self.pred_heatmap_cat[:, n:]
        if self.is_limb:
            self.pred_limb_heatmap_left, self.pred_limb_heatmap_right = left, right
        else:
            self.pred_heatmap_left, self.pred_heatmap_right = left, right

    def backward_HeatMap(self):
        """lambda * (MSE(left) + MSE(right)); limb maps are divided by sqrt(gt_plength) first (heatmap_shared_model.py:109-151)"""
        from . import hm_ops as H
        lam = getattr(self.opt, "lambda_rot_heatmap" if self.is_limb else "lambda_heatmap", 1.0)
        pred = self.pred_heatmap_cat
        gl, dl = H.mse_halves(pred.detach().contiguous(), self._gt, self._plen, lam)
        a, b = self.loss_names
        setattr(self, "loss_" + a, gl[0])
        setattr(self, "loss_" + b, gl[1])
        pred.backward(dl)

    def optimize_parameters(self):
        if not self.isTrain:
            raise RuntimeError("optimize_parameters() needs a model created with opt.isTrain = True")
        _spec.hm_check_batch_stats_side(self.net_HeatMap.hm_size, "stage-1 training (optimize_parameters)")
        self.net_HeatMap.train()
        self.optimizer_HeatMap.zero_grad()
        self.forward()
        self.backward_HeatMap()            # data parallel: the gradient all-reduce runs INSIDE the backward, bucket by bucket on the flat
        self.optimizer_HeatMap.step()      # gradient arena (hm_training.HmTrainFn + parallel.GradReducer), as the lifting head's

    def evaluate(self, runnning_average_dict):
        from . import hm_ops as H
        self.net_HeatMap.eval()
        with torch.no_grad():
            self.forward()
            pred = self.pred_heatmap_cat.contiguous()
            for i in range(pred.shape[0]):                      # per-sample metric, as the reference's loop (:174-217)
                gl, _ = H.mse_halves(pred[i:i + 1], self._gt[i:i + 1], self._plen[i:i + 1] if self._plen is not None else None, 1.0)
                runnning_average_dict.update(dict(mse_heatmap=gl[0] + gl[1]))
        return None, self.pred_heatmap_cat, runnning_average_dict

    def set_eval_mode(self):
        self.net_HeatMap.eval()

    save_networks = EgoTAPAutoEncoderModel.save_networks
    load_networks = EgoTAPAutoEncoderModel.load_networks
    load_optimizers = EgoTAPAutoEncoderModel.load_optimizers
    get_current_errors = EgoTAPAutoEncoderModel.get_current_errors
    update_learning_rate = EgoTAPAutoEncoderModel.update_learning_rate
