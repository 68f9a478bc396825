"""CPU-only: the host state of the seeded device noise (switch_nerf_amd/noise.py behind SwitchNeRF, DenseNeRF, BackgroundScene and
moe.MoELayer), driven through the PUBLIC methods only on host-resident fp32 models (tests/test_optim_tail_cpu.py::_build's kind).

EXPECTED holds literal values, written down from a run of run_all() on the commit BEFORE the state moved into noise.DeviceNoise (four
hand-written attribute sets; the counter was then the private step attribute of each holder, which is why the driver takes the
accessor).  They are not to be regenerated from the code under test.

One record per call: [call, result, states].  result = the return value, or "ErrorType: message" (first 72 characters).  states = one
string per object "name seed/step/base on|off|na counter": seed / step / base as noise_state_dict() gives them, the device_noise
property (na: the layer has none), and the counter tensor after the call - none, same (the object it was before the call) or new.
Further entries of a record are identities between counters that a scenario names (fg_shares_scene, fg_has_own)."""
import types

import pytest
import torch

import synth

SMALL = dict(layer_dim=64, layers=2, skip_layers=(1,), pos_xyz_dim=3, pos_dir_dim=2, appearance_dim=8, appearance_count=10, xyz_dim=3)
OFF, ON = dict(seed=None, step=0, ray_base=0), dict(seed=5, step=6, ray_base=7)


class _Log:
    def __init__(self, counter, objs, **identities):
        self.counter, self.objs, self.identities, self.records = counter, objs, identities, []

    def __call__(self, label, fn, *a, **k):
        before = {n: self.counter(o) for n, o in self.objs.items()}
        try:
            res = fn(*a, **k)
        except (ValueError, RuntimeError, NotImplementedError) as e:
            res = ("%s: %s" % (type(e).__name__, e))[:72]
        states = []
        for n, o in self.objs.items():
            sd, now = o.noise_state_dict(), self.counter(o)
            base = sd["row_base"] if "row_base" in sd else sd["ray_base"]
            on = getattr(o, "device_noise", None)
            states.append("%s %s/%s/%s %s %s" % (n, sd["seed"], sd["step"], base, "na" if on is None else "on" if on else "off",
                                                 "none" if now is None else "same" if now is before[n] else "new"))
        self.records.append([label, res, states] + ["%s=%s" % (k_, f()) for k_, f in self.identities.items()])


def _dense(cfg=SMALL):
    from switch_nerf_amd.dense import DenseNeRF
    return DenseNeRF(cfg, dtype=torch.float32, device="cpu")


def _scene():
    from switch_nerf_amd.background import BackgroundScene
    fg, bg = _dense(), _dense(dict(SMALL, xyz_dim=4))
    return BackgroundScene(fg, bg, synth.SPHERE_CENTER, synth.SPHERE_RADIUS), fg, bg


def _hp(**kw):
    return types.SimpleNamespace(**kw)


def _model_cycle(counter, m):
    log = _Log(counter, dict(m=m))
    log("on(7,3,5)", m.set_device_noise, 7, 3, 5)
    log("off", m.set_device_noise, None)
    log("on(8,2^32-1,1)", m.set_device_noise, 8, (1 << 32) - 1, 1)
    log("ray_base(4)", m.set_ray_base, 4)
    log("load(off)", m.load_noise_state_dict, OFF)
    log("load(on)", m.load_noise_state_dict, ON)
    log("seed=-1", m.set_device_noise, -1)
    log("seed=2^64", m.set_device_noise, 1 << 64)
    log("ray_base=-1", m.set_device_noise, 1, 0, -1)
    log("step=2^32", m.set_device_noise, 1, 1 << 32)
    log("set_ray_base(-1)", m.set_ray_base, -1)
    log("load({})", m.load_noise_state_dict, {})
    log("set_ray_base(-1) off", m.set_ray_base, -1)
    return log.records


def _render_switch(counter):
    """rendering._device_noise on a model's own noise: set_ray_base before and after the switch-on through hparams.device_noise_seed,
    hparams.ray_base overriding and not, a seed change restarting the step at 0 and keeping the base."""
    from switch_nerf_amd import rendering
    from switch_nerf_amd.model import SwitchNeRF
    m = SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")
    log, dn = _Log(counter, dict(m=m)), rendering._device_noise
    log("hp() off", dn, m, None, _hp())
    log("ray_base(768)", m.set_ray_base, 768)
    log("hp(seed=9)", dn, m, None, _hp(device_noise_seed=9))
    log("hp(seed=9) again", dn, m, None, _hp(device_noise_seed=9))
    log("ray_base(256)", m.set_ray_base, 256)
    log("hp(seed=9, ray_base=None)", dn, m, None, _hp(device_noise_seed=9, ray_base=None))
    log("hp(seed=9, ray_base=5)", dn, m, None, _hp(device_noise_seed=9, ray_base=5))
    log("hp(seed=9)", dn, m, None, _hp(device_noise_seed=9))
    log("hp() on", dn, m, None, _hp())
    log("load(10,4,5)", m.load_noise_state_dict, dict(seed=10, step=4, ray_base=5))
    log("hp(seed=10)", dn, m, None, _hp(device_noise_seed=10))
    log("hp(seed=11)", dn, m, None, _hp(device_noise_seed=11))
    log("hp(seed=11) bg_nerf", dn, m, object(), _hp(device_noise_seed=11))
    log("off", m.set_device_noise, None)
    log("ray_base(3) off", m.set_ray_base, 3)
    log("hp(seed=11, ray_base=None)", dn, m, None, _hp(device_noise_seed=11, ray_base=None))
    log("off", m.set_device_noise, None)
    log("hp(seed=12, ray_base=2)", dn, m, None, _hp(device_noise_seed=12, ray_base=2))
    return log.records


def _scene_cycle(counter):
    """Scene on over a model that had its own noise (3, 4, 9), the scene's set_ray_base, a second switch-on with another seed, detach():
    the model reads (3, 4, 9) and holds its original tensor."""
    sc, fg, bg = _scene()
    fg.set_device_noise(3, 4, 9)
    own = counter(fg)
    log = _Log(counter, dict(scene=sc, fg=fg, bg=bg), fg_shares_scene=lambda: counter(fg) is counter(sc) and counter(sc) is not None,
               fg_has_own=lambda: counter(fg) is own)
    log("scene.ray_base(5) off", sc.set_ray_base, 5)
    log("scene.on(11,2,6)", sc.set_device_noise, 11, 2, 6)
    log("scene.ray_base(20)", sc.set_ray_base, 20)
    log("scene.on(12,1,7)", sc.set_device_noise, 12, 1, 7)
    log("scene.seed=-1", sc.set_device_noise, -1)
    log("scene.seed=2^64", sc.set_device_noise, 1 << 64)
    log("scene.ray_base=-1", sc.set_device_noise, 1, 0, -1)
    log("scene.step=2^32", sc.set_device_noise, 1, 1 << 32)
    log("scene.set_ray_base(-1)", sc.set_ray_base, -1)
    log("detach", sc.detach)
    log("scene.load(on)", sc.load_noise_state_dict, ON)
    log("scene.load(off)", sc.load_noise_state_dict, OFF)
    log("scene.on(13)", sc.set_device_noise, 13)
    log("fg.off", fg.set_device_noise, None)
    log("scene.off", sc.set_device_noise, None)
    log("scene.off again", sc.set_device_noise, None)
    return log.records


def _check_sources(counter):
    """Each _check_noise_sources error by message; every case with a model set_device_noise made after the scene's, once with the
    scene's seed (11) and once with another (12)."""
    out = []
    for later in (None, 11, 12):
        for case in ("bg_on", "scene_off", "scene_on"):
            sc, fg, bg = _scene()
            log = _Log(counter, dict(scene=sc, fg=fg, bg=bg), fg_shares_scene=lambda: counter(fg) is counter(sc) and counter(sc) is not None)
            log("scene.on(11,2,6)", sc.set_device_noise, 11, 2, 6)
            if case == "scene_off":
                log("scene.off", sc.set_device_noise, None)
            if later is not None:
                log("fg.on(%d,5,1)" % later, fg.set_device_noise, later, 5, 1)
            elif case == "scene_on":
                log("fg.off", fg.set_device_noise, None)
            if case == "bg_on":
                log("bg.on(5)", bg.set_device_noise, 5)
            log("check %s" % case, sc._check_noise_sources)
            out += log.records
    return out


def _render_scene_carried(counter):
    from switch_nerf_amd import rendering
    sc, fg, bg = _scene()
    log, dn = _Log(counter, dict(scene=sc, fg=fg)), rendering._device_noise
    log("scene.on(11,2,6)", sc.set_device_noise, 11, 2, 6)
    log("hp()", dn, fg, None, _hp())
    log("hp(seed=9)", dn, fg, None, _hp(device_noise_seed=9))
    log("hp(seed=11) bg_nerf", dn, fg, bg, _hp(device_noise_seed=11))
    log("fg.off", fg.set_device_noise, None)
    log("hp() fg off", dn, fg, None, _hp())
    log("hp(seed=9) fg off", dn, fg, None, _hp(device_noise_seed=9))
    log("scene.off", sc.set_device_noise, None)
    log("hp() scene off", dn, fg, None, _hp())
    log("hp(seed=9) scene off", dn, fg, None, _hp(device_noise_seed=9))
    return log.records


def _layer(counter):
    from switch_nerf_amd.moe import MoELayer
    layer = MoELayer(dict(type="top", k=1, capacity_factor=1.0, gate_noise=1.0), 64, dict(type="expertmlp", count_per_node=4, layer_num=2),
                     seeds=(1, 1, 1), dtype=torch.float32)
    log = _Log(counter, dict(layer=layer))
    log("on(99,4,10)", layer.set_device_noise, 99, step=4, row_base=10, device="cpu")
    log("off", layer.set_device_noise, None)
    log("on(98,0,0)", layer.set_device_noise, 98, device="cpu")
    log("load(off)", layer.load_noise_state_dict, dict(seed=None, step=0, row_base=0))
    log("load(on)", layer.load_noise_state_dict, dict(seed=5, step=6, row_base=7))
    log("seed=-1", layer.set_device_noise, -1, device="cpu")
    log("seed=2^64", layer.set_device_noise, 1 << 64, device="cpu")
    log("row_base=-1", layer.set_device_noise, 1, 0, -1, "cpu")
    log("step=2^32", layer.set_device_noise, 1, 1 << 32, 0, "cpu")
    return log.records


def run_all(counter):
    """counter(obj) -> the holder's step-counter tensor (or None before the first switch-on)."""
    from switch_nerf_amd.model import SwitchNeRF
    return dict(moe_cycle=_model_cycle(counter, SwitchNeRF(synth.BUILDING, dtype=torch.float32, device="cpu")),
                dense_cycle=_model_cycle(counter, _dense()), render_switch=_render_switch(counter), scene_cycle=_scene_cycle(counter),
                check_sources=_check_sources(counter), render_scene_carried=_render_scene_carried(counter), layer=_layer(counter))


# written down from the parent of the commit that added switch_nerf_amd/noise.py (see the module doc); the MoE and the dense model gave
# the same records
_CYCLE = [
    ['on(7,3,5)', None, ['m 7/3/5 on new']],
    ['off', None, ['m None/0/0 off same']],
    ['on(8,2^32-1,1)', None, ['m 8/4294967295/1 on same']],
    ['ray_base(4)', None, ['m 8/4294967295/4 on same']],
    ['load(off)', None, ['m None/0/0 off same']],
    ['load(on)', None, ['m 5/6/7 on same']],
    ['seed=-1', 'ValueError: device noise: seed -1 outside [0, 2^64)', ['m 5/6/7 on same']],
    ['seed=2^64', 'ValueError: device noise: seed 18446744073709551616 outside [0, 2^64)', ['m 5/6/7 on same']],
    ['ray_base=-1', 'ValueError: device noise: ray_base -1 < 0', ['m 5/6/7 on same']],
    ['step=2^32', 'ValueError: device noise: step 4294967296 outside [0, 2^32)', ['m 5/6/7 on same']],
    ['set_ray_base(-1)', 'ValueError: device noise: ray_base -1 < 0', ['m 5/6/7 on same']],
    ['load({})', None, ['m None/0/0 off same']],
    ['set_ray_base(-1) off', 'ValueError: device noise: ray_base -1 < 0', ['m None/0/0 off same']],
]
EXPECTED = {
    "moe_cycle": _CYCLE,
    "dense_cycle": _CYCLE,
    "render_switch": [
        ['hp() off', False, ['m None/0/0 off none']],
        ['ray_base(768)', None, ['m None/0/0 off none']],
        ['hp(seed=9)', True, ['m 9/0/768 on new']],
        ['hp(seed=9) again', True, ['m 9/0/768 on same']],
        ['ray_base(256)', None, ['m 9/0/256 on same']],
        ['hp(seed=9, ray_base=None)', True, ['m 9/0/256 on same']],
        ['hp(seed=9, ray_base=5)', True, ['m 9/0/5 on same']],
        ['hp(seed=9)', True, ['m 9/0/5 on same']],
        ['hp() on', True, ['m 9/0/5 on same']],
        ['load(10,4,5)', None, ['m 10/4/5 on same']],
        ['hp(seed=10)', True, ['m 10/4/5 on same']],
        ['hp(seed=11)', True, ['m 11/0/5 on same']],
        ['hp(seed=11) bg_nerf', 'NotImplementedError: device_noise_seed with a background model (bg_nerf)', ['m 11/0/5 on same']],
        ['off', None, ['m None/0/0 off same']],
        ['ray_base(3) off', None, ['m None/0/0 off same']],
        ['hp(seed=11, ray_base=None)', True, ['m 11/0/3 on same']],
        ['off', None, ['m None/0/0 off same']],
        ['hp(seed=12, ray_base=2)', True, ['m 12/0/2 on same']],
    ],
    "scene_cycle": [
        ['scene.ray_base(5) off', None, ['scene None/0/0 off none', 'fg 3/4/9 on same', 'bg None/0/0 off none'], 'fg_shares_scene=False',
         'fg_has_own=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.ray_base(20)', None, ['scene 11/2/20 on same', 'fg 11/2/20 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True',
         'fg_has_own=False'],
        ['scene.on(12,1,7)', None, ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True',
         'fg_has_own=False'],
        ['scene.seed=-1', 'ValueError: device noise: seed -1 outside [0, 2^64)',
         ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.seed=2^64', 'ValueError: device noise: seed 18446744073709551616 outside [0, 2^64)',
         ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.ray_base=-1', 'ValueError: device noise: ray_base -1 < 0', ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'],
         'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.step=2^32', 'ValueError: device noise: step 4294967296 outside [0, 2^32)',
         ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.set_ray_base(-1)', 'ValueError: device noise: ray_base -1 < 0',
         ['scene 12/1/7 on same', 'fg 12/1/7 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['detach', None, ['scene None/0/0 off same', 'fg 3/4/9 on new', 'bg None/0/0 off none'], 'fg_shares_scene=False', 'fg_has_own=True'],
        ['scene.load(on)', None, ['scene 5/6/7 on same', 'fg 5/6/7 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.load(off)', None, ['scene None/0/0 off same', 'fg 3/4/9 on new', 'bg None/0/0 off none'], 'fg_shares_scene=False',
         'fg_has_own=True'],
        ['scene.on(13)', None, ['scene 13/0/0 on same', 'fg 13/0/0 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['fg.off', None, ['scene 13/0/0 on same', 'fg None/0/0 off same', 'bg None/0/0 off none'], 'fg_shares_scene=True', 'fg_has_own=False'],
        ['scene.off', None, ['scene None/0/0 off same', 'fg 3/4/9 on new', 'bg None/0/0 off none'], 'fg_shares_scene=False', 'fg_has_own=True'],
        ['scene.off again', None, ['scene None/0/0 off same', 'fg 3/4/9 on same', 'bg None/0/0 off none'], 'fg_shares_scene=False',
         'fg_has_own=True'],
    ],
    "check_sources": [
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['bg.on(5)', None, ['scene 11/2/6 on same', 'fg 11/2/6 on same', 'bg 5/0/0 on new'], 'fg_shares_scene=True'],
        ['check bg_on', "RuntimeError: BackgroundScene: the background model's own device noise i",
         ['scene 11/2/6 on same', 'fg 11/2/6 on same', 'bg 5/0/0 on same'], 'fg_shares_scene=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['scene.off', None, ['scene None/0/0 off same', 'fg None/0/0 off none', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['check scene_off', None, ['scene None/0/0 off same', 'fg None/0/0 off none', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['fg.off', None, ['scene 11/2/6 on same', 'fg None/0/0 off same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['check scene_on', "RuntimeError: BackgroundScene: the foreground model's device noise was c",
         ['scene 11/2/6 on same', 'fg None/0/0 off same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['fg.on(11,5,1)', None, ['scene 11/5/6 on same', 'fg 11/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['bg.on(5)', None, ['scene 11/5/6 on same', 'fg 11/5/1 on same', 'bg 5/0/0 on new'], 'fg_shares_scene=True'],
        ['check bg_on', "RuntimeError: BackgroundScene: the background model's own device noise i",
         ['scene 11/5/6 on same', 'fg 11/5/1 on same', 'bg 5/0/0 on same'], 'fg_shares_scene=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['scene.off', None, ['scene None/0/0 off same', 'fg None/0/0 off none', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['fg.on(11,5,1)', None, ['scene None/0/0 off same', 'fg 11/5/1 on new', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['check scene_off', "RuntimeError: BackgroundScene: the foreground model's device noise is on",
         ['scene None/0/0 off same', 'fg 11/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['fg.on(11,5,1)', None, ['scene 11/5/6 on same', 'fg 11/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['check scene_on', None, ['scene 11/5/6 on same', 'fg 11/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['fg.on(12,5,1)', None, ['scene 11/5/6 on same', 'fg 12/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['bg.on(5)', None, ['scene 11/5/6 on same', 'fg 12/5/1 on same', 'bg 5/0/0 on new'], 'fg_shares_scene=True'],
        ['check bg_on', "RuntimeError: BackgroundScene: the background model's own device noise i",
         ['scene 11/5/6 on same', 'fg 12/5/1 on same', 'bg 5/0/0 on same'], 'fg_shares_scene=True'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['scene.off', None, ['scene None/0/0 off same', 'fg None/0/0 off none', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['fg.on(12,5,1)', None, ['scene None/0/0 off same', 'fg 12/5/1 on new', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['check scene_off', "RuntimeError: BackgroundScene: the foreground model's device noise is on",
         ['scene None/0/0 off same', 'fg 12/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=False'],
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['fg.on(12,5,1)', None, ['scene 11/5/6 on same', 'fg 12/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
        ['check scene_on', "RuntimeError: BackgroundScene: the foreground model's device noise was c",
         ['scene 11/5/6 on same', 'fg 12/5/1 on same', 'bg None/0/0 off none'], 'fg_shares_scene=True'],
    ],
    "render_scene_carried": [
        ['scene.on(11,2,6)', None, ['scene 11/2/6 on new', 'fg 11/2/6 on new']],
        ['hp()', False, ['scene 11/2/6 on same', 'fg 11/2/6 on same']],
        ['hp(seed=9)', "RuntimeError: device_noise_seed: this model's noise is carried by a Back", ['scene 11/2/6 on same', 'fg 11/2/6 on same']],
        ['hp(seed=11) bg_nerf', "RuntimeError: device_noise_seed: this model's noise is carried by a Back",
         ['scene 11/2/6 on same', 'fg 11/2/6 on same']],
        ['fg.off', None, ['scene 11/2/6 on same', 'fg None/0/0 off same']],
        ['hp() fg off', False, ['scene 11/2/6 on same', 'fg None/0/0 off same']],
        ['hp(seed=9) fg off', "RuntimeError: device_noise_seed: this model's noise is carried by a Back",
         ['scene 11/2/6 on same', 'fg None/0/0 off same']],
        ['scene.off', None, ['scene None/0/0 off same', 'fg None/0/0 off none']],
        ['hp() scene off', False, ['scene None/0/0 off same', 'fg None/0/0 off none']],
        ['hp(seed=9) scene off', True, ['scene None/0/0 off same', 'fg 9/0/0 on new']],
    ],
    "layer": [
        ['on(99,4,10)', None, ['layer 99/4/10 na new']],
        ['off', None, ['layer None/0/0 na same']],
        ['on(98,0,0)', None, ['layer 98/0/0 na same']],
        ['load(off)', None, ['layer None/0/0 na same']],
        ['load(on)', None, ['layer 5/6/7 na same']],
        ['seed=-1', 'ValueError: device noise: seed outside [0, 2^64) or row_base < 0', ['layer 5/6/7 na same']],
        ['seed=2^64', 'ValueError: device noise: seed outside [0, 2^64) or row_base < 0', ['layer 5/6/7 na same']],
        ['row_base=-1', 'ValueError: device noise: seed outside [0, 2^64) or row_base < 0', ['layer 5/6/7 na same']],
        ['step=2^32', 'ValueError: device noise: step 4294967296 outside [0, 2^32)', ['layer 5/6/7 na same']],
    ],
}


@pytest.fixture(scope="module")
def got():
    return run_all(lambda o: o.noise.step)


@pytest.mark.parametrize("name", ["moe_cycle", "dense_cycle", "render_switch", "scene_cycle", "check_sources", "render_scene_carried", "layer"])
def test_noise_host_state(name, got):
    assert got[name] == EXPECTED[name]
