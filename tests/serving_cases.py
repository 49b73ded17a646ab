"""The serving cases of tests/golden/serving_launches.json: what tools/record_serving_launches.py records and test_gpu_serving_launches.py replays.

A case is one request on the shared serving model (gpu_util.serving_model) at B = 3 with opt.hm_chunk = 2 -- one full piece and one ragged piece, the
smallest batch that has both -- and records the (role, kernel, launches) list of the timing hook and a SHA-256 of every returned tensor's bytes.
Groups share the model's state: (heatmap side, precision setting); within a group every entry runs with every output set."""
import hashlib

import torch

from gpu_util import serving_model, timed_launches

B, CHUNK = 3, 2
GROUPS = [(64, "f32"), (64, "bf16"), (64, "bf16_frozen"), (32, "f32"), (32, "bf16")]
ENTRIES = ("rgb", "camera", "sensor")
OUTPUTS = {
    "none": {},
    "keypoints": dict(return_keypoints=True),
    "keypoints_limbs": dict(return_keypoints=True, return_limbs=True),
    "heatmaps": dict(return_heatmaps=True),
}
SENSOR_H, SENSOR_W = 96, 80
SENSOR_ARGS = dict(crop=(4, 2, 72, 90), crop_right=(0, 6, 76, 88), mirror_right=True)


def group_id(hm, setting):
    return f"hm{hm}-{setting}"


def case_id(hm, setting, entry, outputs):
    return f"{group_id(hm, setting)}/{entry}/{outputs}"


def _bytes8(seed, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).cuda()


def _request(m, hm, entry):
    """the entry's bound method and its frames: bytes from a seeded generator; the float entry reads the camera's bytes through the camera table"""
    S0 = 4 * hm
    if entry == "sensor":
        l8, r8 = _bytes8(1, SENSOR_H, SENSOR_W), _bytes8(2, SENSOR_H, SENSOR_W)
        return lambda **kw: m.predict_pose_from_sensor(l8, r8, **SENSOR_ARGS, **kw)
    l8, r8 = _bytes8(3, S0, S0), _bytes8(4, S0, S0)
    if entry == "camera":
        return lambda **kw: m.predict_pose_from_camera(l8, r8, **kw)
    table = m.camera_table(l8.device)
    planes = torch.arange(3, device=l8.device).view(1, 1, 1, 3)
    lf, rf = (table[planes, t.long()].permute(0, 3, 1, 2).contiguous() for t in (l8, r8))
    return lambda **kw: m.predict_pose_from_rgb(lf, rf, **kw)


def _sha256(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run_group(hm, setting):
    """{case id: (launch list, [sha256 of each returned tensor])} of the group's 12 cases; leaves the model as serving_model() hands it out"""
    m, p = serving_model("UnrealEgo", hm)
    got = {}
    try:
        m.set_precision(setting.split("_")[0])
        if setting.endswith("_frozen"):
            assert m.freeze_weights(batch=CHUNK) == {}
        m.opt.hm_chunk = CHUNK
        m._rgb_state(torch.device("cuda", torch.cuda.current_device()))            # (the handle the timing hook sits on)
        for entry in ENTRIES:
            call = _request(m, hm, entry)
            for name, kw in OUTPUTS.items():
                out = []
                launches = timed_launches(m, lambda: out.append(call(**kw)))
                tensors = out[0] if isinstance(out[0], tuple) else (out[0],)
                got[case_id(hm, setting, entry, name)] = ([list(x) for x in launches], [_sha256(t) for t in tensors])
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")
        m.opt.hm_chunk = 256
    return got
