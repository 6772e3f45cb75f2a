"""float64 restatement of the fused backward step (csrc/step_kernels.hip, etainv_eta_backward_step_ex) for n_img image pairs, built from
oracle.schedule the way oracle/loop.py builds eta_variance_noise and step_backward: the reference of tests/test_small_kernels_gpu.py.
tests/test_step_ref.py pins it, without a GPU, against the goldens recorded from the reference implementation."""
import numpy as np
import torch

from oracle import schedule as sch

G = 7.5


def eta_backward_step_ref(x, eps_all, g, x_prev, noise, eta, mask_map, thres, use_mask, ac, t, S, target_dirinv=0.0, dirinv_map=None, dtype=torch.float64):
    """x [2B][c][h][w] (rows src.., tgt..), eps_all [4B][c][h][w] (rows u_s.., u_t.., c_s.., c_t..), x_prev [B][c][h][w], noise [n_cand][c][h][w],
    mask_map / dirinv_map [B][h][w] or None.  use_mask 0: eta everywhere and the source row replayed exactly; 1: eta where mask_map > thres
    (thres as the fp32 value the kernel receives); 2: eta * mask_map.  dirinv_map is the multiplier of the leaked correction (1 - mask_dirinv).
    Returns out_x [2B], out_eps [2B], best [B] (int64), losses [B][n_cand] in `dtype`: float64 is the reference; float32 is the same arithmetic in the
    precision of the kernel, whose distance from the float64 result says what fp32 can resolve (how the tests size a bound that rtol cannot express)."""
    f64 = lambda v: None if v is None else v.detach().cpu().to(dtype)
    x, eps_all, x_prev, noise, mask_map, dirinv_map = map(f64, (x, eps_all, x_prev, noise, mask_map, dirinv_map))
    B = x_prev.shape[0]
    eta, t = float(eta), int(t)
    std = eta * sch.variance(ac, t, S) ** 0.5
    out_x, out_eps = torch.empty_like(x), torch.empty_like(x)
    best, losses = torch.zeros(B, dtype=torch.int64), torch.empty(B, noise.shape[0], dtype=dtype)
    for i in range(B):
        lat = torch.stack([x[i], x[B + i]])
        eps = torch.stack([eps_all[r * B + i] + g * (eps_all[(2 + r) * B + i] - eps_all[r * B + i]) for r in range(2)])    # eta_inversion.py:328
        # eta_inversion.py:330-375 (oracle/loop.py eta_variance_noise): the noise that would reproduce the stored latent, nearest candidate
        mean = sch.ddim_eta_step(lat[:1], eps[:1], ac, t, S, eta, noise=None)
        with np.errstate(all="ignore"):
            opt = (x_prev[i][None] - mean) / torch.tensor(std, dtype=dtype)
        losses[i] = torch.square(noise - opt).reshape(noise.shape[0], -1).mean(1)
        best[i] = int(torch.argmin(losses[i]))
        z = noise[best[i]]
        # eta_inversion.py:207-273 (oracle/loop.py step_backward)
        eta_map = torch.full_like(z, eta)
        if use_mask == 1:
            eta_map = (mask_map[i] > float(np.float32(thres))).to(dtype)[None] * eta_map
        elif use_mask == 2:
            eta_map = mask_map[i][None] * eta_map
        new = sch.ddim_eta_step(lat, eps, ac, t, S, eta_map, noise=z)
        if use_mask:
            delta = x_prev[i] - new[0]
            new[0] = new[0] + delta
            if target_dirinv:
                md = 1.0 if dirinv_map is None else dirinv_map[i][None]
                new[1] = new[1] + target_dirinv * md * delta
        else:
            new[0] = x_prev[i]
        out_x[i], out_x[B + i] = new[0], new[1]
        out_eps[i], out_eps[B + i] = eps[0], eps[1]
    return out_x, out_eps, best, losses


# ---- the golden cases of tests/golden/eta_step*.npz as arguments of eta_backward_step_ref (the preparation tests/test_kernels_gpu.py gives the kernel)
def _shape_mask(m, mode):
    """get_mask tail (eta_inversion.py:196-201)"""
    m = m.float()
    if mode.get("thres", 0.2) is not None:
        m = (m > mode.get("thres", 0.2)).float()
    if mode.get("pow") is not None:
        m = torch.pow(m, mode["pow"])
    return m


def golden_case(name):
    """-> (golden file, keyword arguments of eta_backward_step_ref) for a case of recipes.ETA_CASES / ETA_MODE_CASES / ETA_DIRINV_CASES"""
    from tests.golden import recipes
    inp = recipes.eta_case_inputs(name)
    ac = sch.alphas_cumprod()
    kw = dict(x=inp["latent"].float(), eps_all=inp["unet_out"].float(), g=G, x_prev=inp["src_prev"].float(), noise=inp["noise"].float().reshape(10, 4, 64, 64),
              ac=ac, S=50, thres=0.2)
    paper = [[0.6, 0], [1, 0.7]]
    if name in recipes.ETA_CASES:
        eta_spec, t, _, use_mask = recipes.ETA_CASES[name]
        kw.update(eta=float(sch.eta_table(eta_spec)[t]), t=t, mask_map=inp["mask_map"].float(), use_mask=int(use_mask))
        return "eta_step", kw
    if name in recipes.ETA_MODE_CASES:
        kw.update(eta=float(sch.eta_table(paper)[980]), t=980, mask_map=_shape_mask(inp["mask_map"], recipes.ETA_MODE_CASES[name]), use_mask=2)
        return "eta_step_modes", kw
    mode = recipes.ETA_DIRINV_CASES[name]
    src = {"gt": recipes.dirinv_gt_mask(inp["mask_map"]), "fwd": inp["mask_map"], "fwd_mean": inp["mask_map"]}
    kw.update(eta=float(sch.eta_table(paper)[980]), t=980, mask_map=_shape_mask(src[mode["mask_eta"]], mode), use_mask=2, thres=0.0,
              target_dirinv=float(mode["target_dirinv"]),
              dirinv_map=(1 - _shape_mask(src[mode["mask_dirinv"]], mode)) if mode.get("mask_dirinv") else None)
    return "eta_step_dirinv", kw
