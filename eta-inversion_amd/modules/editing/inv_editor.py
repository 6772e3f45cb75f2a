"""Reconstruction only (reference modules/editing/inv_editor.py:9-53): invert under the source prompt and sample under it alone -- the route by
which an inverter's reconstruction is measured; `vae_rec` returns the VAE round trip instead.  The target prompt is not used."""
from .editor import Editor


class InversionEditor(Editor):
    def __init__(self, inverter, no_source_backward: bool = False, vae_rec: bool = False, no_null_source_prompt: bool = True) -> None:
        # no_null_source_prompt False: the inversion runs under the empty prompt instead of the source prompt (:43)
        self.inverter, self.model = inverter, inverter.model
        self.no_source_backward, self.vae_rec, self.no_null_source_prompt = no_source_backward, vae_rec, no_null_source_prompt

    def edit(self, image, source_prompt, target_prompt, cfg=None):
        assert cfg is None
        if self.vae_rec:
            latent = self.inverter.encode(image)
            return {"image": self.inverter.decode(latent), "latent": latent}
        src_context = self.inverter.create_context(source_prompt if self.no_null_source_prompt else "")
        inv_res = self.inverter.invert(image, context=src_context)
        edit_res = self.inverter.sample(inv_res, context=[src_context])
        return {"image": edit_res["image"], "latent": edit_res["latent"]}
