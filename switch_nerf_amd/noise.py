"""The host state of the seeded device noise (csrc/philox.hpp): SwitchNeRF, BackgroundScene and moe.MoELayer each hold one DeviceNoise.
`step` is created on the first switch-on and afterwards only ever filled - captured launches hold its address; a training step ends in
ONE advance of it.  A BackgroundScene lends its state to the foreground model (lend): a copy with a seed and a base of its own and the
SAME counter, so a model-level re-seed never changes the scene's seed silently; the scene keeps the model's own object and puts it back."""
from . import ops


class DeviceNoise:
    def __init__(self):
        self.seed = None         # None: off
        self.base = 0            # global index of the holder's first ray (a layer: row); on a model it survives a switch-off
        self.step = None         # the step counter: a device int64[1] (the kernels read it, swn_rng_advance bumps it)
        self.owner = None        # the background.BackgroundScene that lent this state to a foreground model, if any

    @property
    def on(self) -> bool:
        return self.seed is not None

    def set(self, seed, step, base, device):
        """Switch on with (seed, step, base) - the counter tensor is made on `device` the first time - or, with seed = None, off."""
        if seed is None:
            self.seed = None
            return
        seed, base = int(seed), int(base)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"device noise: seed {seed} outside [0, 2^64)")
        if base < 0:
            raise ValueError(f"device noise: ray_base {base} < 0")
        step = ops.rng_check_step(step)
        if self.step is None:
            self.step = ops.rng_step_tensor(step, device)
        else:
            self.step.fill_(step)          # (the same tensor: captured launches hold its address)
        self.seed, self.base = seed, base

    def set_base(self, base: int):
        if int(base) < 0:
            raise ValueError(f"device noise: ray_base {base} < 0")
        self.base = int(base)

    def state_dict(self, base_key="ray_base") -> dict:
        """{"seed", "step", base_key}; reads the step back from the device.  Off: seed None, step 0, base 0."""
        if not self.on:
            return {"seed": None, "step": 0, base_key: 0}
        return {"seed": self.seed, "step": int(self.step.item()), base_key: self.base}

    def draw(self, stream_id: int, n: int, elem_base: int, kind: int, scale: float = 1.0):
        """n draws of a stream from global element elem_base on -> f32 [n] (swn_rng_fill; consumed through the supplied-noise arguments)."""
        return ops.rng_fill(n, elem_base, kind, self.seed, self.step, stream_id, scale)

    def advance(self):
        """The step counter's advance: the LAST launch of a training step (inside a captured step).  Nothing when off."""
        if self.on:
            ops.rng_advance(self.step)

    def rewind(self, step: int):
        """Put the counter back behind a capture's warm-up steps (the caller synchronizes).  Nothing when off."""
        if self.on:
            self.step.fill_(step)

    def lend(self, owner):
        """-> a new DeviceNoise with this seed and base, the SAME counter tensor, and `owner` set."""
        lent = DeviceNoise()
        lent.seed, lent.base, lent.step, lent.owner = self.seed, self.base, self.step, owner
        return lent
