"""Per-clip scale-invariant signal-to-distortion ratio (Le Roux et al., "SDR -- half-baked or well done?", 2019), the usual figure of
source separation (extension: the reference has no separation task and no such metric):

    SI-SDR(s, s_hat) = 10 log10(||a s||^2 / ||s_hat - a s||^2),   a = <s_hat, s> / ||s||^2

so rescaling the estimate changes nothing.  Taken in float64 and clamped to [-max_db, max_db] (default 100 dB, far past what fp32 audio
resolves): an estimate that is an exact multiple of the reference scores max_db instead of +inf or a rounding-noise figure, an estimate
orthogonal to the reference -max_db.  A silent reference or a silent estimate gives NaN."""
import numpy as np


class ScaleInvariantSDR:
    def __init__(self, reduction=None, max_db=100.0):
        if reduction not in (None, "mean"):
            raise AssertionError("reduction must be None (per clip) or 'mean'")
        self.reduction, self.max_db = reduction, float(max_db)

    def score(self, reference, estimate):
        """Both arguments: sequences of 1-D clips (lengths may differ; each pair is compared on its common prefix) -> float64 array of dB,
        one per clip.  Two (B, L) CUDA tensors are scored on the GPU (a (B,) float64 CUDA tensor out)."""
        if getattr(reference, "is_cuda", False) and getattr(estimate, "is_cuda", False):
            import torch
            n = min(reference.shape[-1], estimate.shape[-1])
            s, e = reference.double()[..., :n].reshape(-1, n), estimate.double()[..., :n].reshape(-1, n)
            ss = (s * s).sum(dim=1)
            target = ((e * s).sum(dim=1) / ss)[:, None] * s
            db = 10.0 * (torch.log10((target * target).sum(dim=1)) - torch.log10(((e - target) ** 2).sum(dim=1)))
            db = torch.where(ss > 0, db.clamp(-self.max_db, self.max_db), torch.full_like(db, float("nan")))
            return db.mean() if self.reduction == "mean" else db
        out = []
        for s, e in zip(reference, estimate):
            s, e = np.asarray(s, dtype=np.float64).reshape(-1), np.asarray(e, dtype=np.float64).reshape(-1)
            n = min(len(s), len(e))
            s, e = s[:n], e[:n]
            ss = float(np.dot(s, s))
            if not ss > 0:
                out.append(float("nan"))
                continue
            target = (np.dot(e, s) / ss) * s
            with np.errstate(divide="ignore"):
                db = 10.0 * (np.log10(np.dot(target, target)) - np.log10(np.dot(e - target, e - target)))
            out.append(float(np.clip(db, -self.max_db, self.max_db)))
        out = np.asarray(out, dtype=np.float64)
        return out.mean() if self.reduction == "mean" else out
