"""Registries of the reference's modules/__init__.py:31-111: load_inverter / load_editor / get_inversion_methods /
get_edit_methods / register_editor.  Built on the MI355X engine: `etainv`, `dirinv`, `edict`, `regdiffinv`, `npi`, `proxnpi`, `ddpminv`, `cyclediff` (+ the plain `diffinv`
base) and the `simple`, `ptp`, `masactrl`, `pnp`, `invedit` editors; the reference's other method names (`nti`, `pix2pix_zero`: both need gradients
through the UNet) are listed but raise a clear error."""
from functools import partial
from typing import Callable, List

from .inversion.diffusion_inversion import DiffusionInversion
from .inversion.eta_inversion import EtaInversion
from .inversion.direct_inversion import DirectInversion
from .inversion.edict_inversion import EdictInversion
from .inversion.regularized_diffusion_inversion import RegularizedDiffusionInversion
from .inversion.negative_prompt_inversion import NegativePromptInversion
from .inversion.proximal_negative_prompt_inversion import ProximalNegativePromptInversion
from .inversion.ddpm_inversion import DDPMInversion
from .editing.editor import Editor
from .editing.simple_editor import SimpleEditor
from .editing.ptp_editor import PromptToPromptEditor
from .editing.masactrl_editor import MasactrlEditor
from .editing.pnp_editor import PlugAndPlayEditor
from .editing.inv_editor import InversionEditor
from .models import StablePreprocess, StablePostProc, load_diffusion_model


def _not_built(name, *a, **k):
    raise NotImplementedError(f"'{name}' is outside the MI355X hot path built so far (SURVEY.md 8f); available: etainv, dirinv, edict, regdiffinv, npi, proxnpi, "
                              f"ddpminv, cyclediff, diffinv / simple, ptp, masactrl, pnp, invedit")


_inverters = {"diffinv": DiffusionInversion, "etainv": EtaInversion, "dirinv": DirectInversion, "edict": EdictInversion,
              "regdiffinv": RegularizedDiffusionInversion, "npi": NegativePromptInversion, "proxnpi": ProximalNegativePromptInversion,
              "ddpminv": DDPMInversion, "cyclediff": partial(DDPMInversion, markovian_forward=True),
              **{n: partial(_not_built, n) for n in ("nti",)}}
_editors = {"simple": SimpleEditor, "ptp": PromptToPromptEditor, "masactrl": MasactrlEditor, "pnp": PlugAndPlayEditor,
            "invedit": InversionEditor, **{n: partial(_not_built, n) for n in ("pix2pix_zero",)}}


def register_editor(name: str, editor_cls: Callable) -> None:
    print(f"Registering editor {name}")
    _editors[name] = editor_cls


def get_inversion_methods() -> List[str]:
    return list(_inverters.keys())


def get_edit_methods() -> List[str]:
    return list(_editors.keys())


def load_inverter(type: str, **kwargs) -> DiffusionInversion:
    return _inverters[type](**kwargs)


def load_editor(type: str, **kwargs) -> Editor:
    return _editors[type](**kwargs)
