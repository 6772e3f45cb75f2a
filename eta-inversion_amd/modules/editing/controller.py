"""Controller callbacks (reference modules/editing/controller.py:8-110): begin / end / begin_step / end_step / copy, and the wrapper that gives
each member of an EDICT latent pair its own copy of a controller."""
from typing import Optional


class ControllerBase:
    def begin(self) -> None:
        pass

    def end(self) -> None:
        pass

    def begin_step(self, latent, *args, **kwargs):
        return latent

    def end_step(self, latent, noise_pred=None, t: Optional[int] = None):
        return latent

    def copy(self, **kwargs) -> "ControllerBase":
        raise NotImplementedError


class ControllerEmpty(ControllerBase):
    def copy(self, **kwargs) -> "ControllerEmpty":
        return self


class EdictController(ControllerBase):
    """Two copies of a controller, one per member of the EDICT latent pair; `begin_step` selects the copy by `latent_idx` and `end_step`
    goes to the copy selected last (reference :71-110).

    The reference gives every copy its own attention store; the engine has ONE store, which both halves of a step write.  A controller
    that reads the store back -- prompt-to-prompt with LocalBlend (`blend_words`) -- would blend from maps of both pair members, so it is
    refused here rather than computed differently; so is a controller without `copy` (MasaCtrl, user controllers that do not define it)."""

    def __init__(self, controller: ControllerBase) -> None:
        try:
            self.controllers = [controller.copy(latent_idx=i) for i in range(2)]
        except NotImplementedError:
            raise NotImplementedError(f"{type(controller).__name__} has no copy(): the edict inverter runs one controller per member of its "
                                      "latent pair (built: the simple editor, and ptp without blend_words)") from None
        for c in self.controllers:
            if getattr(getattr(c, "controller", None), "local_blend", None) is not None:
                raise NotImplementedError("prompt-to-prompt LocalBlend (blend_words) under the edict inverter needs a per-latent map store: the "
                                          "engine keeps one attention-map store, which both members of the latent pair write")
        self.cur_latent_idx = None

    def begin(self) -> None:
        for c in self.controllers:
            c.begin()

    def end(self) -> None:
        for c in self.controllers:
            c.end()

    def begin_step(self, latent_idx: int, latent_base, latent_model_input) -> None:
        self.cur_latent_idx = latent_idx
        self.controllers[latent_idx].begin_step(latent_base)

    def end_step(self, latent, **kwargs):
        return self.controllers[self.cur_latent_idx].end_step(latent=latent, **kwargs)
