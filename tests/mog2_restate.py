"""cv::BackgroundSubtractorMOG2 restated twice and independently -- plain Python loops over pixels and modes (`impl="loops"`, which also counts the branches it
takes) and vectorised numpy over all pixels at once (`impl="vec"`).  The reference's source (video/src/bgfg_gaussmix2.cpp: MOG2Invoker, detectShadowGMM,
getBackgroundImage_intern) was not available; this text is the definition the kernels of opencv_amd/csrc/mog2.hip are held against, bit for bit.

All arithmetic is IEEE float32, every product, sum and quotient rounded on its own, evaluation left to right.  The model is kept in the reference's order:
modes (h, w) uint8, gmm (h, w, nmixtures, 2) = {weight, variance}, mean (h, w, nmixtures, cn); `export()` zeroes the slots at and above a pixel's count."""
import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)                       # FLT_EPSILON
COUNTERS = ("fit", "fit_swap", "new_mode", "replace_weakest", "prune", "prune_nonlast", "total_eps", "bg_not_first", "shadow_true", "shadow_reject_t", "den0",
            "varmin", "varmax")
DEFAULTS = dict(history=500, nmixtures=5, varThreshold=16.0, backgroundRatio=0.9, varThresholdGen=9.0, varInit=15.0, varMin=4.0, varMax=75.0,
                complexityReductionThreshold=0.05, detectShadows=True, shadowValue=127, shadowThreshold=0.5)


class Mog2:
    def __init__(self, impl="vec", **kw):
        assert impl in ("loops", "vec")
        self.impl = impl
        p = dict(DEFAULTS)
        for k, v in kw.items():
            assert k in p, k
            p[k] = v
        self.p = p
        self.nframes = 0
        self.shape = None
        self.dtype = None
        self.mix_changed = False
        self.modes = self.gmm = self.mean = None
        self.cnt = dict.fromkeys(COUNTERS, 0)

    # ---- parameters (real values are stored as float)
    def set(self, name, v):
        assert name in self.p, name
        self.p[name] = v
        if name == "nmixtures":
            self.mix_changed = True

    def _P(self):
        p = self.p
        return dict(Tb=F(p["varThreshold"]), TB=F(p["backgroundRatio"]), Tg=F(p["varThresholdGen"]), varInit=F(p["varInit"]), varMin=F(p["varMin"]),
                    varMax=F(p["varMax"]), CT=F(p["complexityReductionThreshold"]), tau=F(p["shadowThreshold"]), nmix=int(p["nmixtures"]),
                    shadows=bool(p["detectShadows"]), shadowValue=int(p["shadowValue"]))

    # ---- apply
    def _begin(self, frame, learningRate, may_reinit=True):
        """the re-initialisation rule and the frame's rate alphaT"""
        frame = np.asarray(frame)
        img = frame.reshape(frame.shape[0], frame.shape[1], -1)
        key = img.shape
        if may_reinit and (self.nframes == 0 or learningRate >= 1 or key != self.shape or frame.dtype != self.dtype or self.mix_changed):
            h, w, cn = key
            m = int(self.p["nmixtures"])
            self.shape, self.dtype, self.mix_changed, self.nframes = key, frame.dtype, False, 0
            self.modes = np.zeros((h, w), np.uint8)
            self.gmm = np.zeros((h, w, m, 2), F)
            self.mean = np.zeros((h, w, m, cn), F)
        self.nframes += 1
        lr = learningRate if (learningRate >= 0 and self.nframes > 1) else 1.0 / min(2 * self.nframes, int(self.p["history"]))      # double
        return img.astype(F), F(lr)

    def apply(self, frame, learningRate=-1, _may_reinit=True):
        x, alphaT = self._begin(frame, learningRate, _may_reinit)
        with np.errstate(all="ignore"):
            return (self._apply_loops if self.impl == "loops" else self._apply_vec)(x, alphaT)

    def applyBatch(self, frames, learningRate=-1):
        """frames in time order; learningRate >= 1 or a changed geometry re-initialises before the first frame only"""
        return [self.apply(f, learningRate, _may_reinit=(i == 0)) for i, f in enumerate(frames)]

    def export(self):
        m = self.gmm.shape[2]
        used = np.arange(m)[None, None, :] < self.modes[:, :, None]
        return self.modes.copy(), np.where(used[..., None], self.gmm, F(0)), np.where(used[..., None], self.mean, F(0))

    def getBackgroundImage(self):
        with np.errstate(all="ignore"):
            bg = (self._background_loops if self.impl == "loops" else self._background_vec)()
        h, w, cn = self.shape
        if self.dtype == np.uint8:
            bg = np.clip(np.rint(bg), 0, 255).astype(np.uint8)              # nearest even, saturated
        return bg.reshape(h, w) if cn == 1 else bg

    # ================================================================= loops
    def _apply_loops(self, X, alphaT):
        P, cnt = self._P(), self.cnt
        h, w, cn = self.shape
        nmix = P["nmix"]
        alpha1 = F(1) - alphaT
        prune = -alphaT * P["CT"]
        mask = np.zeros((h, w), np.uint8)
        for yy in range(h):
            for xx in range(w):
                x = [X[yy, xx, c] for c in range(cn)]
                g, mu = self.gmm[yy, xx], self.mean[yy, xx]
                nmodes = int(self.modes[yy, xx])
                background = fits = False
                total = F(0)
                mode = 0
                while mode < nmodes:                                      # the bound is live
                    wgt = alpha1 * g[mode, 0] + prune
                    swaps = 0
                    if not fits:
                        var = g[mode, 1]
                        d = [mu[mode, c] - x[c] for c in range(cn)]
                        dist2 = F(0)
                        for c in range(cn):
                            dist2 = dist2 + d[c] * d[c]
                        if total < P["TB"] and dist2 < P["Tb"] * var:
                            background = True
                            if mode > 0:
                                cnt["bg_not_first"] += 1
                        if dist2 < P["Tg"] * var:
                            fits = True
                            cnt["fit"] += 1
                            wgt = wgt + alphaT
                            k = alphaT / wgt
                            for c in range(cn):
                                mu[mode, c] = mu[mode, c] - k * d[c]
                            v = var + k * (dist2 - var)
                            if not v > P["varMin"]:
                                v = P["varMin"]
                                cnt["varmin"] += 1
                            if not v < P["varMax"]:
                                v = P["varMax"]
                                cnt["varmax"] += 1
                            g[mode, 1] = v
                            i = mode
                            while i > 0:
                                if wgt < g[i - 1, 0]:
                                    break
                                swaps += 1
                                g[[i, i - 1]] = g[[i - 1, i]]
                                mu[[i, i - 1]] = mu[[i - 1, i]]
                                i -= 1
                            if swaps:
                                cnt["fit_swap"] += 1
                    if wgt < -prune:
                        wgt = F(0)
                        cnt["prune"] += 1
                        if mode < nmodes - 1:
                            cnt["prune_nonlast"] += 1
                        nmodes -= 1
                    g[mode - swaps, 0] = wgt
                    total = total + wgt
                    mode += 1
                if abs(total) > EPS:
                    inv = F(1) / total
                else:
                    inv = F(0)
                    cnt["total_eps"] += 1
                for m in range(nmodes):
                    g[m, 0] = g[m, 0] * inv
                if not fits and alphaT > 0:
                    if nmodes == nmix:
                        mode = nmix - 1
                        cnt["replace_weakest"] += 1
                    else:
                        mode = nmodes
                        nmodes += 1
                        cnt["new_mode"] += 1
                    if nmodes == 1:
                        g[mode, 0] = F(1)
                    else:
                        g[mode, 0] = alphaT
                        for i in range(nmodes - 1):
                            g[i, 0] = g[i, 0] * alpha1
                    for c in range(cn):
                        mu[mode, c] = x[c]
                    g[mode, 1] = P["varInit"]
                    i = nmodes - 1
                    while i > 0:
                        if alphaT < g[i - 1, 0]:
                            break
                        g[[i, i - 1]] = g[[i - 1, i]]
                        mu[[i, i - 1]] = mu[[i - 1, i]]
                        i -= 1
                self.modes[yy, xx] = nmodes
                if background:
                    mask[yy, xx] = 0
                elif P["shadows"] and self._shadow_loops(x, nmodes, g, mu, P):
                    mask[yy, xx] = P["shadowValue"]
                else:
                    mask[yy, xx] = 255
        return mask

    def _shadow_loops(self, x, nmodes, g, mu, P):
        cnt = self.cnt
        t = F(0)
        for mode in range(nmodes):
            num = den = F(0)
            for c in range(len(x)):
                num = num + x[c] * mu[mode, c]
                den = den + mu[mode, c] * mu[mode, c]
            if den == 0:
                cnt["den0"] += 1
                return False
            if num <= den and num >= P["tau"] * den:
                a = num / den
                dist2a = F(0)
                for c in range(len(x)):
                    dd = a * mu[mode, c] - x[c]
                    dist2a = dist2a + dd * dd
                if dist2a < P["Tb"] * g[mode, 1] * a * a:
                    cnt["shadow_true"] += 1
                    return True
            t = t + g[mode, 0]
            if t > P["TB"]:
                cnt["shadow_reject_t"] += 1
                return False
        return False

    def _background_loops(self):
        P = self._P()
        h, w, cn = self.shape
        out = np.zeros((h, w, cn), F)
        for yy in range(h):
            for xx in range(w):
                m = [F(0)] * cn
                t = F(0)
                for mode in range(int(self.modes[yy, xx])):
                    wgt = self.gmm[yy, xx, mode, 0]
                    for c in range(cn):
                        m[c] = m[c] + wgt * self.mean[yy, xx, mode, c]
                    t = t + wgt
                    if t > P["TB"]:
                        break
                inv = F(1) / t if abs(t) > EPS else F(0)
                for c in range(cn):
                    out[yy, xx, c] = m[c] * inv
        return out

    # ================================================================= vectorised
    def _apply_vec(self, X, alphaT):
        P = self._P()
        h, w, cn = self.shape
        nmix, N = P["nmix"], h * w
        idx = np.arange(N)
        x = X.reshape(N, cn)
        W = np.ascontiguousarray(self.gmm.reshape(N, nmix, 2)[:, :, 0].T)            # (nmix, N)
        V = np.ascontiguousarray(self.gmm.reshape(N, nmix, 2)[:, :, 1].T)
        MU = np.ascontiguousarray(self.mean.reshape(N, nmix, cn).transpose(1, 0, 2))  # (nmix, N, cn)
        n = self.modes.reshape(N).astype(np.int64)
        alpha1 = F(1) - alphaT
        prune = -alphaT * P["CT"]
        nprune = -prune

        def swap_rows(a, b, sel):
            for A in (W, V):
                ta, tb = A[a].copy(), A[b].copy()
                A[a] = np.where(sel, tb, ta)
                A[b] = np.where(sel, ta, tb)
            ta, tb = MU[a].copy(), MU[b].copy()
            MU[a] = np.where(sel[:, None], tb, ta)
            MU[b] = np.where(sel[:, None], ta, tb)

        background = np.zeros(N, bool)
        fits = np.zeros(N, bool)
        total = np.zeros(N, F)
        for mode in range(nmix):
            act = mode < n                                                            # the live count
            wgt = alpha1 * W[mode] + prune
            cand = act & ~fits
            var = V[mode].copy()
            d = MU[mode] - x
            dist2 = np.zeros(N, F)
            for c in range(cn):
                dist2 = dist2 + d[:, c] * d[:, c]
            background |= cand & (total < P["TB"]) & (dist2 < P["Tb"] * var)
            fit = cand & (dist2 < P["Tg"] * var)
            fits |= fit
            wgt = np.where(fit, wgt + alphaT, wgt)
            k = alphaT / wgt
            MU[mode] = np.where(fit[:, None], MU[mode] - k[:, None] * d, MU[mode])
            v = var + k * (dist2 - var)
            v = np.where(v > P["varMin"], v, P["varMin"])
            v = np.where(v < P["varMax"], v, P["varMax"])
            V[mode] = np.where(fit, v, V[mode])
            pos = np.full(N, mode)
            moving = fit.copy()
            for i in range(mode, 0, -1):
                go = moving & ~(wgt < W[i - 1])
                moving = go
                swap_rows(i, i - 1, go)
                pos = np.where(go, i - 1, pos)
            pr = act & (wgt < nprune)
            wgt = np.where(pr, F(0), wgt)
            n = n - pr
            W[pos[act], idx[act]] = wgt[act]
            total = np.where(act, total + wgt, total)
        inv = np.where(np.abs(total) > EPS, F(1) / total, F(0)).astype(F)
        for m in range(nmix):
            W[m] = np.where(m < n, W[m] * inv, W[m])
        if alphaT > 0:
            new = ~fits
            slot = np.where(n == nmix, nmix - 1, n)
            n = np.where(new & (n < nmix), n + 1, n)
            one = n == 1
            for m in range(nmix):
                W[m] = np.where(new & ~one & (m < n - 1), W[m] * alpha1, W[m])
            s, j = slot[new], idx[new]
            W[s, j] = np.where(one[new], F(1), alphaT)
            V[s, j] = P["varInit"]
            MU[s, j] = x[new]
            moving = new.copy()
            for i in range(nmix - 1, 0, -1):
                elig = moving & (i <= n - 1)
                go = elig & ~(alphaT < W[i - 1])
                moving = moving & ~(elig & ~go)
                swap_rows(i - 1, i, go)
        self.modes[...] = n.reshape(h, w).astype(np.uint8)
        self.gmm[...] = np.stack([W.T, V.T], axis=-1).reshape(h, w, nmix, 2)
        self.mean[...] = MU.transpose(1, 0, 2).reshape(h, w, nmix, cn)
        mask = np.full(N, 255, np.uint8)
        if P["shadows"]:
            mask[self._shadow_vec(x, n, W, V, MU, P)] = P["shadowValue"]
        mask[background] = 0
        return mask.reshape(h, w)

    @staticmethod
    def _shadow_vec(x, n, W, V, MU, P):
        N, cn = x.shape
        res = np.zeros(N, bool)
        done = np.zeros(N, bool)
        t = np.zeros(N, F)
        for mode in range(W.shape[0]):
            live = (mode < n) & ~done
            num = np.zeros(N, F)
            den = np.zeros(N, F)
            for c in range(cn):
                num = num + x[:, c] * MU[mode, :, c]
                den = den + MU[mode, :, c] * MU[mode, :, c]
            zero = live & (den == 0)
            done |= zero
            live &= ~zero
            inside = live & (num <= den) & (num >= P["tau"] * den)
            a = num / den
            dist2a = np.zeros(N, F)
            for c in range(cn):
                dd = a * MU[mode, :, c] - x[:, c]
                dist2a = dist2a + dd * dd
            hit = inside & (dist2a < P["Tb"] * V[mode] * a * a)
            res |= hit
            done |= hit
            live &= ~hit
            t = np.where(live, t + W[mode], t)
            done |= live & (t > P["TB"])
        return res

    def _background_vec(self):
        P = self._P()
        h, w, cn = self.shape
        acc = np.zeros((h, w, cn), F)
        t = np.zeros((h, w), F)
        done = np.zeros((h, w), bool)
        for mode in range(self.gmm.shape[2]):
            live = (mode < self.modes) & ~done
            wgt = self.gmm[:, :, mode, 0]
            acc = np.where(live[..., None], acc + wgt[..., None] * self.mean[:, :, mode, :], acc)
            t = np.where(live, t + wgt, t)
            done |= live & (t > P["TB"])
        inv = np.where(np.abs(t) > EPS, F(1) / t, F(0)).astype(F)
        return acc * inv[..., None]


def same_model(a, b):
    """two exports (modes, gmm, mean) equal bit for bit"""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def sequence(h, w, cn, dtype, seed=0, nframes=22):
    """(frames, rates): a fixed camera over few grey levels that walks through every branch of the update -- a static background with one level of noise (fits, the
    variance falling to varMin), an early step that still fits at a high explicit rate (varMax), a multiplicative dimming (shadows) and a brightening (the shadow loop left
    through t > TB), black pixels (den == 0), six distinct values in a row (more than five modes: the weakest replaced), a fast phase that prunes several weak modes at
    once (a prune that is not the last mode) and one frame at rate 0.95 that prunes everything (total <= FLT_EPSILON).  Use with history <= 8."""
    rng = np.random.default_rng(seed)
    levels = np.array([0, 40, 80, 120, 200], np.float64)
    base = levels[rng.integers(0, len(levels), (h, w, cn))]
    base[0, 0, :] = 0                                                   # a black pixel whatever the draw
    frames, rates = [], []

    def emit(img, rate):
        img = np.clip(img, 0, 255)
        if dtype == np.uint8:
            out = np.rint(img).astype(np.uint8)
        else:
            out = (img + 0.25).astype(np.float32)
        frames.append(out.reshape(h, w) if cn == 1 else out)
        rates.append(rate)

    block = np.zeros((h, w, 1), bool)
    block[h // 3:, w // 3:] = True
    for t in range(nframes):
        noise = rng.integers(-1, 2, (h, w, cn))
        if t == 0:
            emit(base, -1)
        elif t == 1:                                                      # channel 0 steps by 11 while the variance is still varInit: fits, and k is close to 1
            step = np.zeros((1, 1, cn))
            step[0, 0, 0] = 11
            emit(base + np.where(block, step, 0), 0.9)
        elif t < 4:
            emit(base + noise, -1)
        elif t < 6:
            emit(base + np.where(block, 10, 0), 0.9)
        elif t < 8:
            emit(base + noise, 0.05)
        elif t < 10:
            emit(np.where(block, base * 0.6, base * 1.5 + 30), 0.05)
        elif t < 16:
            emit(np.where(block, (base + 37 * (t - 9)) % 256, base + noise), 0.1)
        elif t < 18:
            emit(base + noise, 0.5)
        elif t == 18:
            emit((base + 101) % 256, 0.95)
        else:
            emit(base + noise, -1)
    return frames, rates
