"""numpy / scipy restatement of constraint_learning_by_obseration (src/constraint_learning_by_observation.jl:8-163): float64
accumulation over the TF values the reference's own arithmetic produces, with its quirks (*_min / *_LB start at 1e8 in float64,
*_max / *_UB start at 0 in TF) and this project's documented divergences (a count over all-zero magnitudes is 0, cumulative sums
in float64, wavelet_l1 = 0 unless n1 == n2)."""
import numpy as np
import scipy.fft

from tests import dwt_ref

KEYS = ("nuclear_norm", "nuclear_Dx", "nuclear_Dz", "rank_095", "TV", "wavelet_l1", "Dx_l1", "Dz_l1", "DFT_l1", "DFT_card_095",
        "TV_card_095", "annulus", "TV_annulus", "D_l2", "D_x_min", "D_x_max", "D_z_min", "D_z_max", "DCT_x_LB", "DCT_x_UB",
        "DCT_y_LB", "DCT_y_UB", "hist_min", "hist_max", "hist_TV_min", "hist_TV_max")


def diffs(img, h):
    """D_x img ((n1-1) x n2) and D_z img (n1 x (n2-1)) in TF: (-fl(1/h)) x + fl(1/h) x_next, each product rounded, then the add."""
    TF = img.dtype.type
    ih1, ih2 = TF(1) / TF(h[0]), TF(1) / TF(h[1])
    dx = (-ih1) * img[:-1, :] + ih1 * img[1:, :]
    dz = (-ih2) * img[:, :-1] + ih2 * img[:, 1:]
    return dx, dz


def tv_rows(img, h):
    dx, dz = diffs(img, h)
    return np.concatenate([dz.reshape(-1, order="F"), dx.reshape(-1, order="F")])


def card_095(c):
    """length(c) - findfirst(cumsum(sort(|c|)) / total > 0.05), the cumulative sum in float64; 0 when every |c| is 0."""
    a = np.sort(np.abs(c).astype(np.float64).ravel())
    t = np.cumsum(a)
    if t[-1] == 0:
        return 0, np.inf
    t = t / t[-1]
    k = int(np.argmax(t > 0.05))
    return len(a) - (k + 1), abs(t[k] - 0.05)


def rank_095(s):
    """findfirst(cumsum(sigma) / sum(sigma) > 0.95), 1-based; 0 when sigma = 0."""
    t = np.cumsum(s)
    if t[-1] == 0:
        return 0, np.inf
    t = t / t[-1]
    k = int(np.argmax(t > 0.95))
    return k + 1, abs(t[k] - 0.95)


def learn(m_train, h, margins=None):
    """The reference's dictionary for images m_train[i] (n_train x n1 x n2).  margins, if a dict, receives per count key the
    distance of the normalised cumulative sum from its threshold at the decisive index, per image."""
    m = np.asarray(m_train)
    if m.ndim == 2:
        m = m[None]
    TF = m.dtype.type
    TI = np.int32 if TF == np.float32 else np.int64
    nt, n1, n2 = m.shape
    N, M = n1 * n2, (n1 - 1) * n2 + n1 * (n2 - 1)
    o = {k: np.zeros(nt, TF) for k in KEYS[:18]}
    for k in ("rank_095", "DFT_card_095", "TV_card_095"):
        o[k] = np.zeros(nt, TI)
    o.update(DCT_x_LB=np.zeros(n1) + 1e8, DCT_x_UB=np.zeros(n1, TF), DCT_y_LB=np.zeros(n2) + 1e8, DCT_y_UB=np.zeros(n2, TF),
             hist_min=np.zeros(N) + 1e8, hist_max=np.zeros(N, TF), hist_TV_min=np.zeros(M) + 1e8, hist_TV_max=np.zeros(M, TF))
    mg = {k: np.zeros(nt) for k in ("rank_095", "DFT_card_095", "TV_card_095")}
    f64 = lambda a: np.asarray(a, np.float64)
    for i in range(nt):
        img = m[i]
        v = img.reshape(-1, order="F")
        dx, dz = diffs(img, h)
        tv = tv_rows(img, h)
        o["hist_min"] = np.minimum(o["hist_min"], np.sort(v))
        o["hist_max"] = np.maximum(o["hist_max"], np.sort(v))
        o["hist_TV_min"] = np.minimum(o["hist_TV_min"], np.sort(tv))
        o["hist_TV_max"] = np.maximum(o["hist_TV_max"], np.sort(tv))
        sv = np.linalg.svd(f64(img), compute_uv=False)
        o["nuclear_norm"][i] = sv.sum()
        o["nuclear_Dx"][i] = np.linalg.svd(f64(dx), compute_uv=False).sum()
        o["nuclear_Dz"][i] = np.linalg.svd(f64(dz), compute_uv=False).sum()
        o["rank_095"][i], mg["rank_095"][i] = rank_095(sv)
        o["D_x_min"][i], o["D_x_max"][i] = dx.min(), dx.max()
        o["D_z_min"][i], o["D_z_max"][i] = dz.min(), dz.max()
        o["TV"][i] = np.abs(f64(tv)).sum()
        if n1 == n2:
            o["wavelet_l1"][i] = np.abs(dwt_ref.dwt(f64(img))).sum()
        o["Dx_l1"][i] = np.abs(f64(dx)).sum()
        o["Dz_l1"][i] = np.abs(f64(dz)).sum()
        o["D_l2"][i] = o["TV_annulus"][i] = np.sqrt((f64(tv) ** 2).sum())
        o["annulus"][i] = np.sqrt((f64(v) ** 2).sum())
        F = np.fft.fft2(f64(img), norm="ortho")
        o["DFT_l1"][i] = np.abs(F).sum()
        o["DFT_card_095"][i], mg["DFT_card_095"][i] = card_095(F)
        o["TV_card_095"][i], mg["TV_card_095"][i] = card_095(tv)
        cx = scipy.fft.dct(f64(img), type=2, axis=0, norm="ortho")
        o["DCT_x_LB"] = np.minimum(o["DCT_x_LB"], cx.min(axis=1))
        o["DCT_x_UB"] = np.maximum(o["DCT_x_UB"], cx.max(axis=1).astype(TF))
        cy = scipy.fft.dct(f64(img), type=2, axis=1, norm="ortho")
        o["DCT_y_LB"] = np.minimum(o["DCT_y_LB"], cy.min(axis=0))
        o["DCT_y_UB"] = np.maximum(o["DCT_y_UB"], cy.max(axis=0).astype(TF))
    if margins is not None:
        margins.update(mg)
    return o
