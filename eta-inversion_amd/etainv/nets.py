"""SD1.x VAE (AutoencoderKL) and CLIP ViT-L/14 text encoder on the native kernels.

These third-party networks sit outside the DDIM loop (1 encode + 2 decodes + 4 text forwards per image, about 1.5 % of the
FLOPs): the host code below only sequences C-ABI kernel calls (`etainv_op_*`: MFMA implicit-GEMM convs / linears,
GroupNorm, LayerNorm, im2col, row softmax, causal attention) on device buffers.  They replace
`model.vae.encode(...)["latent_dist"].mean`, `model.vae.decode(...)["sample"]` and `model.text_encoder(ids)[0]`
(reference modules/inversion/diffusion_inversion.py:193, 206, 230).  Weights: diffusers / transformers state-dict names."""
import math
import zlib

import torch

from . import _capi
from .weights import synthetic_clip_tensor, synthetic_tensor


def _dev(t, dtype):
    return t.detach().to(device="cuda", dtype=dtype).contiguous()


class _Ops:
    def __init__(self, dtype):
        self.lib, self.dtype, self.code = _capi.load(), dtype, _capi.dtype_code(dtype)
        self._scratch = {}

    def st(self):
        return _capi.stream_ptr()

    def gemm(self, a, w, bias=None, residual=None):
        m, k = a.shape
        n = w.shape[0]
        out = torch.empty(m, n, dtype=self.dtype, device=a.device)
        _capi.check(self.lib.etainv_op_gemm(_capi.ptr(a), _capi.ptr(w), _capi.ptr(bias), _capi.ptr(residual), _capi.ptr(out), m, n, k, 0,
                                            self.code, self.st()))
        return out

    def conv3(self, x, w, bias, stride=1, ups=0, pad0=0, residual=None, out_nchw=0):
        b, h, wd, cin = x.shape
        cout = w.shape[0]
        ho = h * 2 if ups else (h // 2 if stride == 2 else h)
        wo = wd * 2 if ups else (wd // 2 if stride == 2 else wd)
        if out_nchw:
            out = torch.empty(b, out_nchw, ho, wo, dtype=torch.float32, device=x.device)
        else:
            out = torch.empty(b, ho, wo, cout, dtype=self.dtype, device=x.device)
        _capi.check(self.lib.etainv_op_conv3x3_ex(_capi.ptr(x), _capi.ptr(w), _capi.ptr(bias), _capi.ptr(residual), _capi.ptr(out), b, h, wd,
                                                  cin, cout, stride, ups, pad0, out_nchw, _capi.F32, self.code, self.st()))
        return out

    def gn(self, x, gamma, beta, silu, eps=1e-6):
        b, c = x.shape[0], x.shape[-1]
        hw = x.numel() // (b * c)
        out = torch.empty_like(x)
        key = ("gn", b)
        if key not in self._scratch:
            self._scratch[key] = torch.zeros(b * 65 * 64, dtype=torch.float32, device=x.device)
        _capi.check(self.lib.etainv_op_groupnorm(_capi.ptr(x), None, c, 0, _capi.ptr(gamma), _capi.ptr(beta), _capi.ptr(out), b, hw, 32, eps,
                                                 int(silu), _capi.ptr(self._scratch[key]), self.code, self.st()))
        return out

    def ln(self, x, gamma, beta, eps=1e-5):
        rows, c = x.shape
        out = torch.empty_like(x)
        _capi.check(self.lib.etainv_op_layernorm(_capi.ptr(x), _capi.ptr(gamma), _capi.ptr(beta), _capi.ptr(out), rows, c, eps, self.code, self.st()))
        return out

    def im2col(self, x_nchw, premix=None):
        b, cin, h, w = x_nchw.shape
        x_nchw = x_nchw.float().contiguous()
        out = torch.empty(b * h * w, 64, dtype=self.dtype, device=x_nchw.device)
        _capi.check(self.lib.etainv_op_im2col3x3(_capi.ptr(x_nchw), _capi.F32, cin, h, w, b, _capi.ptr(premix), _capi.ptr(out), self.code, self.st()))
        return out


def _pack_conv3(w):                       # [O][I][3][3] -> [O][9][I]
    return w.permute(0, 2, 3, 1).contiguous()


def _pack_conv_small(w):                  # [O][cin<=4][3][3] -> [O][64], k = tap*cin + ci
    o, cin = w.shape[:2]
    out = torch.zeros(o, 64)
    out[:, : 9 * cin] = w.permute(0, 2, 3, 1).reshape(o, 9 * cin)
    return out


class NativeVAE:
    dtype = torch.float32   # boundary dtype (images / latents are fp32 at the boundary)

    def __init__(self, state_dict=None, compute_dtype=torch.float16, seed=0):
        self.ops = _Ops(compute_dtype)
        self.cd = compute_dtype
        self._sd, self._seed = state_dict, seed
        self.w = {}
        self._build()

    def _get(self, name, shape):
        if self._sd is not None:
            t = self._sd[name].float()
            assert tuple(t.shape) == tuple(shape), (name, t.shape, shape)
            return t
        return synthetic_tensor("vae." + name, shape, self._seed)

    def _res(self, prefix, cin, cout):
        g = self._get
        d = {"n1": (_dev(g(prefix + ".norm1.weight", (cin,)), torch.float32), _dev(g(prefix + ".norm1.bias", (cin,)), torch.float32)),
             "c1": (_dev(_pack_conv3(g(prefix + ".conv1.weight", (cout, cin, 3, 3))), self.cd), _dev(g(prefix + ".conv1.bias", (cout,)), torch.float32)),
             "n2": (_dev(g(prefix + ".norm2.weight", (cout,)), torch.float32), _dev(g(prefix + ".norm2.bias", (cout,)), torch.float32)),
             "c2": (_dev(_pack_conv3(g(prefix + ".conv2.weight", (cout, cout, 3, 3))), self.cd), _dev(g(prefix + ".conv2.bias", (cout,)), torch.float32)),
             "sc": None}
        if cin != cout:
            d["sc"] = (_dev(g(prefix + ".conv_shortcut.weight", (cout, cin, 1, 1)).reshape(cout, cin), self.cd),
                       _dev(g(prefix + ".conv_shortcut.bias", (cout,)), torch.float32))
        return d

    def _attn(self, prefix, c):
        g = self._get
        lin = lambda n, bias=True: (_dev(g(f"{prefix}.{n}.weight", (c, c)), self.cd), _dev(g(f"{prefix}.{n}.bias", (c,)), torch.float32))
        return {"gn": (_dev(g(prefix + ".group_norm.weight", (c,)), torch.float32), _dev(g(prefix + ".group_norm.bias", (c,)), torch.float32)),
                "q": lin("to_q"), "k": lin("to_k"), "v": lin("to_v"), "o": lin("to_out.0")}

    def _conv(self, prefix, c):
        return (_dev(_pack_conv3(self._get(prefix + ".weight", (c, c, 3, 3))), self.cd), _dev(self._get(prefix + ".bias", (c,)), torch.float32))

    def _build(self):
        g, ch = self._get, (128, 256, 512, 512)
        e, d = {}, {}
        e["conv_in"] = (_dev(_pack_conv_small(g("encoder.conv_in.weight", (128, 3, 3, 3))), self.cd), _dev(g("encoder.conv_in.bias", (128,)), torch.float32))
        cin = ch[0]
        e["down"] = []
        for i, c in enumerate(ch):
            blk = {"res": [self._res(f"encoder.down_blocks.{i}.resnets.0", cin, c), self._res(f"encoder.down_blocks.{i}.resnets.1", c, c)],
                   "down": self._conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c) if i < 3 else None}
            e["down"].append(blk)
            cin = c
        e["mid"] = (self._res("encoder.mid_block.resnets.0", 512, 512), self._attn("encoder.mid_block.attentions.0", 512),
                    self._res("encoder.mid_block.resnets.1", 512, 512))
        e["norm_out"] = (_dev(g("encoder.conv_norm_out.weight", (512,)), torch.float32), _dev(g("encoder.conv_norm_out.bias", (512,)), torch.float32))
        # conv_out (512 -> 8 moments) followed by the 1x1 quant_conv; only the 4 mean channels are needed: fold both
        w_out, b_out = g("encoder.conv_out.weight", (8, 512, 3, 3)), g("encoder.conv_out.bias", (8,))
        q, qb = g("quant_conv.weight", (8, 8, 1, 1)).reshape(8, 8), g("quant_conv.bias", (8,))
        w_mean = torch.einsum("oc,cikl->oikl", q[:4], w_out)
        b_mean = q[:4] @ b_out + qb[:4]
        e["conv_out"] = (_dev(_pack_conv3(w_mean), self.cd), _dev(b_mean, torch.float32))
        # decoder
        pq, pqb = g("post_quant_conv.weight", (4, 4, 1, 1)).reshape(4, 4), g("post_quant_conv.bias", (4,))
        d["premix"] = _dev(torch.cat([pq, pqb[:, None]], 1), torch.float32)
        d["conv_in"] = (_dev(_pack_conv_small(g("decoder.conv_in.weight", (512, 4, 3, 3))), self.cd), _dev(g("decoder.conv_in.bias", (512,)), torch.float32))
        d["mid"] = (self._res("decoder.mid_block.resnets.0", 512, 512), self._attn("decoder.mid_block.attentions.0", 512),
                    self._res("decoder.mid_block.resnets.1", 512, 512))
        rev, cin = (512, 512, 256, 128), 512
        d["up"] = []
        for i, c in enumerate(rev):
            blk = {"res": [self._res(f"decoder.up_blocks.{i}.resnets.0", cin, c), self._res(f"decoder.up_blocks.{i}.resnets.1", c, c),
                           self._res(f"decoder.up_blocks.{i}.resnets.2", c, c)],
                   "up": self._conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c) if i < 3 else None}
            d["up"].append(blk)
            cin = c
        d["norm_out"] = (_dev(g("decoder.conv_norm_out.weight", (128,)), torch.float32), _dev(g("decoder.conv_norm_out.bias", (128,)), torch.float32))
        w3 = torch.zeros(4, 128, 3, 3)
        w3[:3] = g("decoder.conv_out.weight", (3, 128, 3, 3))
        b3 = torch.zeros(4)
        b3[:3] = g("decoder.conv_out.bias", (3,))
        d["conv_out"] = (_dev(_pack_conv3(w3), self.cd), _dev(b3, torch.float32))
        self.enc, self.dec = e, d

    # ------------------------------------------------------------------ blocks
    def _run_res(self, r, x):
        o = self.ops
        h = o.conv3(o.gn(x, *r["n1"], True), *r["c1"])
        res = x
        if r["sc"] is not None:
            b, hh, ww, c = x.shape
            res = o.gemm(x.reshape(b * hh * ww, c), *r["sc"]).reshape(b, hh, ww, -1)
        return o.conv3(o.gn(h, *r["n2"], True), *r["c2"], residual=res)

    def _run_attn(self, a, x):
        o = self.ops
        b, hh, ww, c = x.shape
        n = hh * ww
        assert n % 64 == 0, "VAE attention needs H*W to be a multiple of 64"
        t = o.gn(x, *a["gn"], False).reshape(b, n, c)
        q = o.gemm(t.reshape(b * n, c), *a["q"]).reshape(b, n, c)
        k = o.gemm(t.reshape(b * n, c), *a["k"]).reshape(b, n, c)
        outs = []
        for i in range(b):                                                    # scores materialised once per image
            s = o.gemm(q[i], k[i])                                            # [n][n] = Q K^T
            _capi.check(o.lib.etainv_op_row_softmax(_capi.ptr(s), n, n, c ** -0.5, o.code, o.st()))
            vt = o.gemm(a["v"][0], t[i])                                      # [c][n] = (X Wv^T)^T  (bias folded below)
            outs.append(o.gemm(s, vt, a["v"][1]))                             # P V + b_v   (rows of P sum to 1)
        att = torch.stack(outs).reshape(b * n, c)
        return o.gemm(att, *a["o"], residual=x.reshape(b * n, c)).reshape(b, hh, ww, c)

    def _mid(self, m, x):
        return self._run_res(m[2], self._run_attn(m[1], self._run_res(m[0], x)))

    # ------------------------------------------------------------------ API of the reference's `model.vae`
    def encode(self, image):
        """image (B,3,H,W) in [-1,1] -> {"latent_dist": obj with .mean (B,4,H/8,W/8)}"""
        o, e = self.ops, self.enc
        b, _, hh, ww = image.shape
        x = o.gemm(o.im2col(image.cuda()), *e["conv_in"]).reshape(b, hh, ww, 128)
        for blk in e["down"]:
            for r in blk["res"]:
                x = self._run_res(r, x)
            if blk["down"] is not None:
                x = o.conv3(x, *blk["down"], stride=2, pad0=1)
        x = self._mid(e["mid"], x)
        mean = o.conv3(o.gn(x, *e["norm_out"], True), *e["conv_out"], out_nchw=4)

        class _Dist:
            pass
        dist = _Dist()
        dist.mean = mean
        return {"latent_dist": dist}

    def decode(self, z):
        """z (B,4,h,w) -> {"sample": (B,3,8h,8w)}"""
        o, d = self.ops, self.dec
        b, _, hh, ww = z.shape
        x = o.gemm(o.im2col(z.cuda(), d["premix"]), *d["conv_in"]).reshape(b, hh, ww, 512)
        x = self._mid(d["mid"], x)
        for blk in d["up"]:
            for r in blk["res"]:
                x = self._run_res(r, x)
            if blk["up"] is not None:
                x = o.conv3(x, *blk["up"], ups=1)
        return {"sample": o.conv3(o.gn(x, *d["norm_out"], True), *d["conv_out"], out_nchw=3)}


class NativeCLIPText:
    def __init__(self, state_dict=None, compute_dtype=torch.float16, seed=0, layers=12, d=768, heads=12, vocab=49408):
        self.ops, self.cd, self.d, self.heads = _Ops(compute_dtype), compute_dtype, d, heads
        self._sd, self._seed = state_dict, seed
        g = self._get
        pre = "text_model."
        self.tok = _dev(g(pre + "embeddings.token_embedding.weight", (vocab, d)), compute_dtype)
        self.pos = _dev(g(pre + "embeddings.position_embedding.weight", (77, d)), compute_dtype)
        f32 = torch.float32
        self.layers = []
        for i in range(layers):
            p = f"{pre}encoder.layers.{i}."
            wq, wk, wv = (g(p + f"self_attn.{n}.weight", (d, d)) for n in ("q_proj", "k_proj", "v_proj"))
            bq, bk, bv = (g(p + f"self_attn.{n}.bias", (d,)) for n in ("q_proj", "k_proj", "v_proj"))
            self.layers.append({
                "ln1": (_dev(g(p + "layer_norm1.weight", (d,)), f32), _dev(g(p + "layer_norm1.bias", (d,)), f32)),
                "qkv": (_dev(torch.cat([wq, wk, wv]), compute_dtype), _dev(torch.cat([bq, bk, bv]), f32)),
                "out": (_dev(g(p + "self_attn.out_proj.weight", (d, d)), compute_dtype), _dev(g(p + "self_attn.out_proj.bias", (d,)), f32)),
                "ln2": (_dev(g(p + "layer_norm2.weight", (d,)), f32), _dev(g(p + "layer_norm2.bias", (d,)), f32)),
                "fc1": (_dev(g(p + "mlp.fc1.weight", (4 * d, d)), compute_dtype), _dev(g(p + "mlp.fc1.bias", (4 * d,)), f32)),
                "fc2": (_dev(g(p + "mlp.fc2.weight", (d, 4 * d)), compute_dtype), _dev(g(p + "mlp.fc2.bias", (d,)), f32))})
        self.final_ln = (_dev(g(pre + "final_layer_norm.weight", (d,)), f32), _dev(g(pre + "final_layer_norm.bias", (d,)), f32))

    def _get(self, name, shape):
        if self._sd is not None:
            t = self._sd[name].float()
            assert tuple(t.shape) == tuple(shape), (name, t.shape, shape)
            return t
        if "embedding" in name:
            g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + 1000003 * self._seed) & 0x7FFFFFFF)
            return 0.5 * torch.randn(shape, generator=g)
        return synthetic_tensor("clip." + name, shape, self._seed)

    def __call__(self, input_ids):
        """(B,77) int64 -> (last_hidden_state (B,77,768) fp32,)   [`text_encoder(ids)[0]`, diffusion_inversion.py:230]"""
        o, d = self.ops, self.d
        ids = input_ids.to(device="cuda", dtype=torch.int64).contiguous()
        b, n = ids.shape
        x = torch.empty(b * n, d, dtype=self.cd, device="cuda")
        _capi.check(o.lib.etainv_op_embed(_capi.ptr(ids), _capi.ptr(self.tok), _capi.ptr(self.pos), b, n, d, _capi.ptr(x), o.code, o.st()))
        for l in self.layers:
            qkv = o.gemm(o.ln(x, *l["ln1"]), *l["qkv"])
            att = torch.empty(b * n, d, dtype=self.cd, device="cuda")
            _capi.check(o.lib.etainv_op_causal_attention(_capi.ptr(qkv), _capi.ptr(att), b, n, self.heads, d // self.heads, o.code, o.st()))
            x = o.gemm(att, *l["out"], residual=x)
            f = o.gemm(o.ln(x, *l["ln2"]), *l["fc1"])
            _capi.check(o.lib.etainv_op_quick_gelu(_capi.ptr(f), _capi.ptr(f), f.numel(), o.code, o.st()))
            x = o.gemm(f, *l["fc2"], residual=x)
        return (o.ln(x, *self.final_ln).reshape(b, n, d).float(),)


class NativeCLIPVision:
    """CLIP's ViT image tower (transformers `CLIPModel` names under `vision_model.`): patch-embedding GEMM on the rows etainv_clip_preprocess
    writes, class token + position embeddings, pre_layrnorm, and the encoder layers of NativeCLIPText with etainv_op_vit_attention in place of the
    causal kernel.  Any width that is a multiple of 64, heads = width / 64.  Returns the encoder's output; post_layernorm runs in the embedding head
    (etainv_clip_embed_head), on the pooled token only."""

    def __init__(self, state_dict=None, compute_dtype=torch.float16, seed=0, layers=12, d=768, patch=16, image=224):
        if d % 64 or patch not in (14, 16, 32) or image % patch:
            raise ValueError(f"NativeCLIPVision: width {d} must be a multiple of 64, patch {patch} one of 14, 16, 32 and divide the image size {image}")
        self.ops, self.cd, self.d, self.heads, self.patch, self.image = _Ops(compute_dtype), compute_dtype, d, d // 64, patch, image
        self._sd, self._seed = state_dict, seed
        g = self._get
        pre = "vision_model."
        f32 = torch.float32
        self.g2 = (image // patch) ** 2
        k = 3 * patch * patch
        self.kp = (k + 63) // 64 * 64
        w = torch.zeros(d, self.kp)
        w[:, :k] = g(pre + "embeddings.patch_embedding.weight", (d, 3, patch, patch)).reshape(d, k)
        self.patch_w = _dev(w, compute_dtype)
        self.cls = _dev(g(pre + "embeddings.class_embedding", (d,)), compute_dtype)
        self.pos = _dev(g(pre + "embeddings.position_embedding.weight", (self.g2 + 1, d)), compute_dtype)
        self.pre_ln = (_dev(g(pre + "pre_layrnorm.weight", (d,)), f32), _dev(g(pre + "pre_layrnorm.bias", (d,)), f32))
        self.layers = []
        for i in range(layers):
            p = f"{pre}encoder.layers.{i}."
            wq, wk, wv = (g(p + f"self_attn.{n}.weight", (d, d)) for n in ("q_proj", "k_proj", "v_proj"))
            bq, bk, bv = (g(p + f"self_attn.{n}.bias", (d,)) for n in ("q_proj", "k_proj", "v_proj"))
            self.layers.append({
                "ln1": (_dev(g(p + "layer_norm1.weight", (d,)), f32), _dev(g(p + "layer_norm1.bias", (d,)), f32)),
                "qkv": (_dev(torch.cat([wq, wk, wv]), compute_dtype), _dev(torch.cat([bq, bk, bv]), f32)),
                "out": (_dev(g(p + "self_attn.out_proj.weight", (d, d)), compute_dtype), _dev(g(p + "self_attn.out_proj.bias", (d,)), f32)),
                "ln2": (_dev(g(p + "layer_norm2.weight", (d,)), f32), _dev(g(p + "layer_norm2.bias", (d,)), f32)),
                "fc1": (_dev(g(p + "mlp.fc1.weight", (4 * d, d)), compute_dtype), _dev(g(p + "mlp.fc1.bias", (4 * d,)), f32)),
                "fc2": (_dev(g(p + "mlp.fc2.weight", (d, 4 * d)), compute_dtype), _dev(g(p + "mlp.fc2.bias", (d,)), f32))})
        self.post_ln = (_dev(g(pre + "post_layernorm.weight", (d,)), f32), _dev(g(pre + "post_layernorm.bias", (d,)), f32))

    def _get(self, name, shape):
        if self._sd is not None:
            t = self._sd[name].float()
            assert tuple(t.shape) == tuple(shape), (name, t.shape, shape)
            return t
        return synthetic_clip_tensor(name, shape, self._seed)

    def __call__(self, rows, b):
        """patch rows [b g^2][Kp] (compute dtype, from etainv_clip_preprocess) -> hidden states [b][1 + g^2][d] (compute dtype)"""
        o, d, n = self.ops, self.d, self.g2 + 1
        assert rows.shape == (b * self.g2, self.kp) and rows.dtype == self.cd, (rows.shape, rows.dtype)
        pe = o.gemm(rows, self.patch_w)
        x = torch.empty(b * n, d, dtype=self.cd, device="cuda")
        _capi.check(o.lib.etainv_clip_assemble_tokens(_capi.ptr(pe), _capi.ptr(self.cls), _capi.ptr(self.pos), _capi.ptr(x), b, self.g2, d, o.code, o.st()))
        x = o.ln(x, *self.pre_ln)
        for l in self.layers:
            qkv = o.gemm(o.ln(x, *l["ln1"]), *l["qkv"])
            att = torch.empty(b * n, d, dtype=self.cd, device="cuda")
            _capi.check(o.lib.etainv_op_vit_attention(_capi.ptr(qkv), _capi.ptr(att), b, n, self.heads, 64, o.code, o.st()))
            x = o.gemm(att, *l["out"], residual=x)
            f = o.gemm(o.ln(x, *l["ln2"]), *l["fc1"])
            _capi.check(o.lib.etainv_op_quick_gelu(_capi.ptr(f), _capi.ptr(f), f.numel(), o.code, o.st()))
            x = o.gemm(f, *l["fc2"], residual=x)
        return x.reshape(b, n, d)


class NativeDinoVision:
    """DINO's ViT (the names of its published checkpoints) up to the keys of its last block: patch-embedding GEMM WITH bias on the rows
    etainv_dino_preprocess writes, class token + position embeddings, then the pre-LN blocks of NativeCLIPVision with LayerNorm eps 1e-6 and the
    erf GELU (etainv_op_gelu_erf); no pre-LayerNorm and no final norm.  The last block runs only norm1 and the key third of its qkv GEMM (weight
    rows d .. 2d-1 with their bias): `blocks[L-1].attn.qkv`'s output columns d .. 2d-1, which is what the reference's hook keeps
    (dino_vit_structure.py:182-189).  heads = d / 64; any depth L >= 1 (the reference asserts L = 12: its models have 12 blocks; the keys are
    those of block L-1 here).  The geometry comes from the tensor shapes (dino_geometry)."""

    def __init__(self, state_dict, compute_dtype=torch.float16):
        gm = dino_geometry(state_dict)
        d, patch, layers = gm["width"], gm["patch"], gm["layers"]
        self.ops, self.cd, self.d, self.heads, self.patch, self.image, self.g2 = _Ops(compute_dtype), compute_dtype, d, d // 64, patch, gm["image"], gm["g2"]
        f32 = torch.float32
        g = lambda name, shape: self._get(state_dict, name, shape)
        self.kp = 3 * patch * patch
        self.patch_w = _dev(g("patch_embed.proj.weight", (d, 3, patch, patch)).reshape(d, self.kp), compute_dtype)
        self.patch_b = _dev(g("patch_embed.proj.bias", (d,)), f32)
        self.cls = _dev(g("cls_token", (1, 1, d)).reshape(d), compute_dtype)
        self.pos = _dev(g("pos_embed", (1, self.g2 + 1, d)).reshape(self.g2 + 1, d), compute_dtype)
        lin = lambda name, o, k: (_dev(g(name + ".weight", (o, k)), compute_dtype), _dev(g(name + ".bias", (o,)), f32))
        ln = lambda name: (_dev(g(name + ".weight", (d,)), f32), _dev(g(name + ".bias", (d,)), f32))
        self.layers = []
        for i in range(layers - 1):
            p = f"blocks.{i}."
            self.layers.append({"ln1": ln(p + "norm1"), "qkv": lin(p + "attn.qkv", 3 * d, d), "out": lin(p + "attn.proj", d, d), "ln2": ln(p + "norm2"),
                                "fc1": lin(p + "mlp.fc1", 4 * d, d), "fc2": lin(p + "mlp.fc2", d, 4 * d)})
        p = f"blocks.{layers - 1}."
        self.last_ln = ln(p + "norm1")
        self.key_w = _dev(g(p + "attn.qkv.weight", (3 * d, d))[d:2 * d], compute_dtype)
        self.key_b = _dev(g(p + "attn.qkv.bias", (3 * d,))[d:2 * d], f32)

    @staticmethod
    def _get(sd, name, shape):
        if name not in sd:
            raise ValueError(f"DINO state dict: {name} missing")
        t = sd[name].float()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"DINO state dict: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def __call__(self, rows, b):
        """patch rows [b g^2][3 p^2] (compute dtype, from etainv_dino_preprocess) -> the last block's keys [b][1 + g^2][d] (compute dtype)"""
        o, d, n = self.ops, self.d, self.g2 + 1
        assert rows.shape == (b * self.g2, self.kp) and rows.dtype == self.cd, (rows.shape, rows.dtype)
        pe = o.gemm(rows, self.patch_w, self.patch_b)
        x = torch.empty(b * n, d, dtype=self.cd, device="cuda")
        _capi.check(o.lib.etainv_clip_assemble_tokens(_capi.ptr(pe), _capi.ptr(self.cls), _capi.ptr(self.pos), _capi.ptr(x), b, self.g2, d, o.code, o.st()))
        for l in self.layers:
            qkv = o.gemm(o.ln(x, *l["ln1"], eps=1e-6), *l["qkv"])
            att = torch.empty(b * n, d, dtype=self.cd, device="cuda")
            _capi.check(o.lib.etainv_op_vit_attention(_capi.ptr(qkv), _capi.ptr(att), b, n, self.heads, 64, o.code, o.st()))
            x = o.gemm(att, *l["out"], residual=x)
            f = o.gemm(o.ln(x, *l["ln2"], eps=1e-6), *l["fc1"])
            _capi.check(o.lib.etainv_op_gelu_erf(_capi.ptr(f), _capi.ptr(f), f.numel(), o.code, o.st()))
            x = o.gemm(f, *l["fc2"], residual=x)
        return o.gemm(o.ln(x, *self.last_ln, eps=1e-6), self.key_w, self.key_b).reshape(b, n, d)


def dino_geometry(state_dict, image=None):
    """the sizes of a DINO ViT state dict, read from its tensor shapes; refuses, with the reason, what the tower is not built for.  `image`: the
    side the model runs at (None: 224, or the model's own side when its position table is smaller -- tiny models)"""
    sd = state_dict
    bad = sorted({part for k in sd for part in k.split(".") if part in ("ls1", "ls2", "gamma_1", "gamma_2", "register_tokens")})
    if bad:
        raise ValueError(f"a DINOv2 state dict ({', '.join(bad)}): LayerScale and register tokens are not built here (dinovitstruct_v2: dinov2_geometry, NativeDinov2Vision)")
    for k in ("patch_embed.proj.weight", "pos_embed", "cls_token"):
        if k not in sd:
            raise ValueError(f"not a DINO ViT state dict: {k} missing")
    w, n_pos = sd["patch_embed.proj.weight"], sd["pos_embed"].shape[-2]
    d, p = w.shape[0], w.shape[-1]
    if d % 64:
        raise ValueError(f"DINO tower: width {d} is not a multiple of 64 (heads of 64 channels)")
    if p not in (8, 16) or w.shape[-2] != p:
        raise ValueError(f"DINO tower: patch size {tuple(w.shape[-2:])} must be 8 x 8 or 16 x 16")
    layers = len({k.split(".")[1] for k in sd if k.startswith("blocks.")})
    if layers < 1:
        raise ValueError("DINO tower: no blocks in the state dict")
    own = math.isqrt(max(n_pos - 1, 0)) * p
    if image is None:
        image = 224 if n_pos == 1 + (224 // p) ** 2 else own
    if n_pos != 1 + (image // p) ** 2 or image % p or image < p:
        raise ValueError(f"DINO tower: pos_embed has {n_pos} rows, expected 1 + ({image} / {p})^2 = {1 + (image // p) ** 2} (the position embeddings are "
                         f"not interpolated: the model runs at the image size it was trained at)")
    return {"width": d, "patch": p, "layers": layers, "image": image, "g2": (image // p) ** 2}


DINOV2_PATCH, DINOV2_KP = 14, 640              # 3 * 14^2 = 588 values per patch row, padded with zeros to a whole number of 64-wide K steps


def dinov2_geometry(state_dict, image=None):
    """the sizes of a DINOv2 ViT state dict, read from its tensor shapes: width, patch (14), layers, `table` (the side M of the position grid:
    37 for the published models, trained at 518), `image` (the side the model runs at; None: 224, or M * 14 when the table is smaller than
    224 / 14 -- tiny models) and g2 = (image / 14)^2.  Refuses, with the reason, what the tower is not built for."""
    sd = state_dict
    if "register_tokens" in sd:
        raise ValueError("DINOv2 tower: register tokens (the dinov2_vit*14_reg models) are not built")
    if any(".mlp.w12." in k for k in sd):
        raise ValueError("DINOv2 tower: the SwiGLU feed-forward of dinov2_vitg14 (mlp.w12, mlp.w3) is not built")
    for k in ("patch_embed.proj.weight", "pos_embed", "cls_token", "blocks.0.ls1.gamma"):
        if k not in sd:
            raise ValueError(f"not a DINOv2 ViT state dict: {k} missing")
    w, n_pos = sd["patch_embed.proj.weight"], sd["pos_embed"].shape[-2]
    d = w.shape[0]
    if d % 64:
        raise ValueError(f"DINOv2 tower: width {d} is not a multiple of 64 (heads of 64 channels)")
    if tuple(w.shape[-2:]) != (DINOV2_PATCH, DINOV2_PATCH):
        raise ValueError(f"DINOv2 tower: patch size {tuple(w.shape[-2:])} must be 14 x 14")
    m = math.isqrt(max(n_pos - 1, 0))
    if m < 1 or n_pos != 1 + m * m:
        raise ValueError(f"DINOv2 tower: pos_embed has {n_pos} rows, which is not 1 + M^2 for a square M x M position table")
    layers = len({k.split(".")[1] for k in sd if k.startswith("blocks.")})
    if image is None:
        image = 224 if m >= 224 // DINOV2_PATCH else m * DINOV2_PATCH
    if image < DINOV2_PATCH or image % DINOV2_PATCH:
        raise ValueError(f"DINOv2 tower: the image side {image} must be a positive multiple of 14")
    return {"width": d, "patch": DINOV2_PATCH, "layers": layers, "table": m, "image": image, "g2": (image // DINOV2_PATCH) ** 2}


def dinov2_position_table(pos_embed, g, interpolate_offset=0.1):
    """pos_embed [1][1 + M^2][d] -> float32 [1 + g^2][d] for a g x g patch grid, as the published DINOv2 `interpolate_pos_encoding` builds it:
    the table as it is when g == M; otherwise, in float32, the M x M patch part through F.interpolate(mode="bicubic", antialias=False) with
    scale_factor (g + offset) / M when `interpolate_offset` is not zero (torch then maps coordinates with 1 / scale_factor, not M / g) or with
    size (g, g) when it is zero (transformers' Dinov2Model), behind the class row unchanged."""
    import torch.nn.functional as F
    pos = pos_embed.detach().float().reshape(-1, pos_embed.shape[-1])
    m, d = math.isqrt(pos.shape[0] - 1), pos.shape[1]
    if g == m:
        return pos.contiguous()
    grid = pos[1:].reshape(1, m, m, d).permute(0, 3, 1, 2)
    if interpolate_offset:
        sf = float(g + interpolate_offset) / m
        out = F.interpolate(grid, mode="bicubic", antialias=False, scale_factor=(sf, sf))
    else:
        out = F.interpolate(grid, mode="bicubic", antialias=False, size=(g, g))
    if tuple(out.shape[-2:]) != (g, g):
        raise ValueError(f"DINOv2 tower: interpolate_offset {interpolate_offset} gives a {tuple(out.shape[-2:])} position grid, not {g} x {g}")
    return torch.cat([pos[:1], out.permute(0, 2, 3, 1).reshape(g * g, d)]).contiguous()


class NativeDinov2Vision:
    """DINOv2's ViT (dinov2_vits14 / vitb14 / vitl14: the names of the published checkpoints) up to the keys of its last block.  Over
    NativeDinoVision: patch 14 on rows of DINOV2_KP = 640 (etainv_dinov2_preprocess; the patch weight is padded with zero columns), a position table
    interpolated ONCE here, on the host, for the grid the model runs at (dinov2_position_table: the call the published model makes), and
    LayerScale: x = x + ls.gamma * branch(x).  The branch's last GEMM runs without residual and etainv_op_layerscale_add_layernorm applies
    gamma in fp32, adds, stores x and writes the NEXT LayerNorm's output in the same pass; gamma is never folded into the 16-bit weights.
    Launches for L blocks: ln (block 0's norm1), then per block qkv, attention, proj, fused (ls1, norm2), fc1, gelu, fc2, fused (ls2, next
    norm1); block L-2's last fusion stores no x; block L-1 is the key third of its qkv GEMM."""

    def __init__(self, state_dict, compute_dtype=torch.float16, interpolate_offset=0.1, image=None):
        import torch.nn.functional as F
        gm = dinov2_geometry(state_dict, image)
        d, layers = gm["width"], gm["layers"]
        self.ops, self.cd, self.d, self.heads, self.patch, self.image, self.g2 = _Ops(compute_dtype), compute_dtype, d, d // 64, 14, gm["image"], gm["g2"]
        self.table, self.interpolate_offset, self.kp = gm["table"], float(interpolate_offset), DINOV2_KP
        f32 = torch.float32
        g = lambda name, shape: self._get(state_dict, name, shape)
        self.patch_w = _dev(F.pad(g("patch_embed.proj.weight", (d, 3, 14, 14)).reshape(d, 588), (0, DINOV2_KP - 588)), compute_dtype)
        self.patch_b = _dev(g("patch_embed.proj.bias", (d,)), f32)
        self.cls = _dev(g("cls_token", (1, 1, d)).reshape(d), compute_dtype)
        self.pos = _dev(dinov2_position_table(g("pos_embed", (1, gm["table"] ** 2 + 1, d)), math.isqrt(self.g2), self.interpolate_offset), compute_dtype)
        lin = lambda name, o, k: (_dev(g(name + ".weight", (o, k)), compute_dtype), _dev(g(name + ".bias", (o,)), f32))
        ln = lambda name: (_dev(g(name + ".weight", (d,)), f32), _dev(g(name + ".bias", (d,)), f32))
        self.first_ln = ln("blocks.0.norm1")
        self.layers = []
        for i in range(layers - 1):
            p = f"blocks.{i}."
            self.layers.append({"qkv": lin(p + "attn.qkv", 3 * d, d), "out": lin(p + "attn.proj", d, d), "ls1": _dev(g(p + "ls1.gamma", (d,)), f32),
                                "ln2": ln(p + "norm2"), "fc1": lin(p + "mlp.fc1", 4 * d, d), "fc2": lin(p + "mlp.fc2", d, 4 * d),
                                "ls2": _dev(g(p + "ls2.gamma", (d,)), f32), "next_ln1": ln(f"blocks.{i + 1}.norm1")})
        p = f"blocks.{layers - 1}."
        self.key_w = _dev(g(p + "attn.qkv.weight", (3 * d, d))[d:2 * d], compute_dtype)
        self.key_b = _dev(g(p + "attn.qkv.bias", (3 * d,))[d:2 * d], f32)

    @staticmethod
    def _get(sd, name, shape):
        if name not in sd:
            raise ValueError(f"DINOv2 state dict: {name} missing")
        t = sd[name].float()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"DINOv2 state dict: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def ls_ln(self, y, ls, x, ln, store_x=True):
        """x <- x + ls * y in place (unless store_x is False) and LayerNorm of the stored sum, one launch; returns the LayerNorm's output"""
        o = self.ops
        h = torch.empty_like(x)
        _capi.check(o.lib.etainv_op_layerscale_add_layernorm(_capi.ptr(y), _capi.ptr(ls), _capi.ptr(x), _capi.ptr(ln[0]), _capi.ptr(ln[1]), 1e-6,
                                                             _capi.ptr(x) if store_x else None, _capi.ptr(h), x.shape[0], x.shape[1], o.code, o.st()))
        return h

    def __call__(self, rows, b):
        """patch rows [b g^2][640] (compute dtype, from etainv_dinov2_preprocess) -> the last block's keys [b][1 + g^2][d] (compute dtype)"""
        o, d, n = self.ops, self.d, self.g2 + 1
        assert rows.shape == (b * self.g2, self.kp) and rows.dtype == self.cd, (rows.shape, rows.dtype)
        pe = o.gemm(rows, self.patch_w, self.patch_b)
        x = torch.empty(b * n, d, dtype=self.cd, device="cuda")
        _capi.check(o.lib.etainv_clip_assemble_tokens(_capi.ptr(pe), _capi.ptr(self.cls), _capi.ptr(self.pos), _capi.ptr(x), b, self.g2, d, o.code, o.st()))
        h = o.ln(x, *self.first_ln, eps=1e-6)
        for i, l in enumerate(self.layers):
            qkv = o.gemm(h, *l["qkv"])
            att = torch.empty(b * n, d, dtype=self.cd, device="cuda")
            _capi.check(o.lib.etainv_op_vit_attention(_capi.ptr(qkv), _capi.ptr(att), b, n, self.heads, 64, o.code, o.st()))
            h = self.ls_ln(o.gemm(att, *l["out"]), l["ls1"], x, l["ln2"])
            f = o.gemm(h, *l["fc1"])
            _capi.check(o.lib.etainv_op_gelu_erf(_capi.ptr(f), _capi.ptr(f), f.numel(), o.code, o.st()))
            h = self.ls_ln(o.gemm(f, *l["fc2"]), l["ls2"], x, l["next_ln1"], store_x=i < len(self.layers) - 1)
        return o.gemm(h, self.key_w, self.key_b).reshape(b, n, d)


def clip_geometry(state_dict):
    """the sizes of a transformers `CLIPModel` state dict, read from its tensor shapes"""
    sd = state_dict
    w = sd["vision_model.embeddings.patch_embedding.weight"]
    g2 = sd["vision_model.embeddings.position_embedding.weight"].shape[0] - 1
    count = lambda pre: len({k.split(".")[3] for k in sd if k.startswith(pre + "encoder.layers.")})
    tok = sd["text_model.embeddings.token_embedding.weight"]
    return {"width": w.shape[0], "layers": count("vision_model."), "patch": w.shape[-1], "image": math.isqrt(g2) * w.shape[-1],
            "proj": sd["visual_projection.weight"].shape[0], "text_width": tok.shape[1], "text_layers": count("text_model."), "vocab": tok.shape[0]}


class NativeCLIP:
    """The two towers of a CLIP model and their projections: unit image and text embeddings (reference metrics/clip_similarity.py:191-221:
    `model.encode_image` / `model.encode_text` divided by their norm)."""

    def __init__(self, state_dict=None, compute_dtype=torch.float16, seed=0, width=768, layers=12, patch=16, image=224, proj=512, text_width=512,
                 text_layers=12, vocab=49408):
        if state_dict is not None:
            gm = clip_geometry(state_dict)
            width, layers, patch, image, proj = gm["width"], gm["layers"], gm["patch"], gm["image"], gm["proj"]
            text_width, text_layers, vocab = gm["text_width"], gm["text_layers"], gm["vocab"]
        self.cd, self.proj, self.patch, self.image, self.vocab = compute_dtype, proj, patch, image, vocab
        self.vision = NativeCLIPVision(state_dict, compute_dtype, seed, layers=layers, d=width, patch=patch, image=image)
        self.text = NativeCLIPText(state_dict, compute_dtype, seed, layers=text_layers, d=text_width, heads=text_width // 64, vocab=vocab)
        get = lambda name, shape: state_dict[name].float() if state_dict is not None else synthetic_clip_tensor(name, shape, seed)
        self.visual_projection = _dev(get("visual_projection.weight", (proj, width)), torch.float32)
        self.text_projection = _dev(get("text_projection.weight", (proj, text_width)), torch.float32)

    def _head(self, x, index, ln, w):
        b, n, d = x.shape
        out = torch.empty(b, self.proj, dtype=torch.float32, device="cuda")
        lib = self.vision.ops.lib
        _capi.check(lib.etainv_clip_embed_head(_capi.ptr(x), _capi.dtype_code(x.dtype), _capi.ptr(index), b, n, d, _capi.ptr(ln[0]) if ln else None,
                                               _capi.ptr(ln[1]) if ln else None, 1e-5, _capi.ptr(w), _capi.F32, self.proj, _capi.ptr(out),
                                               _capi.stream_ptr()))
        return out

    def image_features(self, rows, b):
        """patch rows of b images -> unit embeddings (b, proj) fp32"""
        return self._head(self.vision(rows, b).contiguous(), None, self.vision.post_ln, self.visual_projection)

    def text_features(self, input_ids):
        """(B, 77) int64 -> unit embeddings (B, proj) fp32, pooled at argmax(ids) (the end-of-text token: OpenAI's rule).  The text tower's
        output is already final-LayerNormed: the head applies none."""
        if int(input_ids.max()) >= self.vocab or int(input_ids.min()) < 0:      # (on the host when the ids are there: no device synchronisation)
            raise ValueError(f"token id outside the vocabulary of {self.vocab} entries")
        ids = input_ids.to(device="cuda", dtype=torch.int64)
        hidden = self.text(ids)[0].contiguous()
        return self._head(hidden, ids.argmax(-1).to(torch.int32).contiguous(), None, self.text_projection)


class NativeLpipsAlex:
    """torchvision's AlexNet `features` for LPIPS, tapped after each of its five ReLUs: etainv_op_conv2d_relu (bias and ReLU in the epilogue) and
    etainv_op_maxpool3s2 over NHWC, on the rows etainv_lpips_preprocess writes.  Weights (the names of weights.lpips_shapes) are packed once,
    here, to [cout][kh kw][cin] by etainv_op_pack_weight mode 1 (conv1 with a zero fourth input channel); the `lin` heads stay fp32 [C].  The
    intermediate buffers are allocated once per (n, H, W) and reused, so the taps of a call are valid until the next call with that shape."""

    def __init__(self, state_dict, compute_dtype=torch.float16):
        from .weights import LPIPS_CONVS, LPIPS_KERNELS, lpips_shapes
        self.lib, self.cd, self.code = _capi.load(), compute_dtype, _capi.dtype_code(compute_dtype)
        self.widths = tuple(int(state_dict[f"features.{n}.weight"].shape[0]) for n in LPIPS_CONVS)
        for name, shape in lpips_shapes(self.widths).items():
            if name not in state_dict or tuple(state_dict[name].shape) != tuple(shape):
                raise ValueError(f"LPIPS state dict: {name} missing or not of shape {tuple(shape)}")
        self.convs, self.lins, self._buffers = [], [], {}
        for i, n in enumerate(LPIPS_CONVS):
            w = state_dict[f"features.{n}.weight"].float()
            if i == 0:
                w = torch.cat([w, torch.zeros_like(w[:, :1])], 1)                 # the fourth input channel etainv_lpips_preprocess writes as 0
            cout, cin, k, _ = w.shape
            src, packed = _dev(w, torch.float32), torch.empty(cout, k * k, cin, dtype=compute_dtype, device="cuda")
            _capi.check(self.lib.etainv_op_pack_weight(_capi.ptr(src), _capi.ptr(packed), cout, cin * k * k, 1, k * k, 1.0, None, self.code,
                                                       _capi.stream_ptr()))
            self.convs.append((packed, _dev(state_dict[f"features.{n}.bias"], torch.float32), cin, cout) + LPIPS_KERNELS[i])
            self.lins.append(_dev(state_dict[f"lin{i}.model.1.weight"].reshape(-1), torch.float32))
        torch.cuda.current_stream().synchronize()                                # (the fp32 sources go out of scope)

    @staticmethod
    def tap_sizes(h, w):
        """[(H, W)] of the five taps for an h x w input"""
        c = lambda s, k, st, p: (s + 2 * p - k) // st + 1
        pool = lambda s: (s - 3) // 2 + 1
        t1 = (c(h, 11, 4, 2), c(w, 11, 4, 2))
        t2 = (pool(t1[0]), pool(t1[1]))
        t3 = (pool(t2[0]), pool(t2[1]))
        return [t1, t2, t3, t3, t3]

    def _conv(self, x, out, n, h, w, i):
        wt, bias, cin, cout, k, stride, pad = self.convs[i]
        _capi.check(self.lib.etainv_op_conv2d_relu(_capi.ptr(x), _capi.ptr(wt), _capi.ptr(bias), _capi.ptr(out), n, h, w, cin, cout, k, k, stride, pad, 1,
                                                   self.code, _capi.stream_ptr()))

    def _pool(self, x, out, n, h, w, c):
        _capi.check(self.lib.etainv_op_maxpool3s2(_capi.ptr(x), _capi.ptr(out), n, h, w, c, self.code, _capi.stream_ptr()))

    def __call__(self, x_nhwc4, n):
        """[n][H][W][4] (compute dtype, from etainv_lpips_preprocess) -> the five taps, each [n][pixels][C] in the compute dtype"""
        assert x_nhwc4.dim() == 4 and x_nhwc4.shape[0] == n and x_nhwc4.shape[3] == 4 and x_nhwc4.dtype == self.cd, (x_nhwc4.shape, x_nhwc4.dtype)
        h, w = int(x_nhwc4.shape[1]), int(x_nhwc4.shape[2])
        sizes, wd = self.tap_sizes(h, w), self.widths
        key = (n, h, w, str(x_nhwc4.device))
        if key not in self._buffers:
            new = lambda hw, c: torch.empty(n, hw[0] * hw[1], c, dtype=self.cd, device=x_nhwc4.device)
            self._buffers[key] = ([new(sizes[i], wd[i]) for i in range(5)], new(sizes[1], wd[0]), new(sizes[2], wd[1]))
        taps, p1, p2 = self._buffers[key]
        self._conv(x_nhwc4, taps[0], n, h, w, 0)
        self._pool(taps[0], p1, n, *sizes[0], wd[0])
        self._conv(p1, taps[1], n, *sizes[1], 1)
        self._pool(taps[1], p2, n, *sizes[1], wd[1])
        self._conv(p2, taps[2], n, *sizes[2], 2)
        self._conv(taps[2], taps[3], n, *sizes[2], 3)
        self._conv(taps[3], taps[4], n, *sizes[2], 4)
        return taps
