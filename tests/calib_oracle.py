"""The calibration rule of the reference's reorder_indices.py, restated with torch on the CPU over a list of batches (one batch: one
hooked forward pass, `tensor.view(-1, hidden_dim)`).  Like the reference it keeps every activation until the end (:46, :100); the
tests of micromix_amd.calib's streaming form (include/micromix_calib.h) compare against it.

    thresholds(v, lamda)   the per-row p4 / p6 thresholds of fp32 |x| rows, the reference's expression in fp32 (:103-104)
    split(c4, c6, numel, K)   (p6, p8) from the integer counts in the reference's fp32 tensor arithmetic (:106-110), then the two clamps
                           of calib.split_from_activations
    run(batches, lamda)    everything of one key:
        means      per batch, fp32(fp64 column sum of |x| / rows)
        score64    the maximum over the batches of the fp64 means (NaN from either side stays, torch.max, :47)
        score      the same maximum of `means`: what the device's score equals bit for bit where its partial sums are exact
        score_ref  the reference's own scores: fp32 torch.mean per batch (:44) and their maximum
        count4, count6, numel   (:106-107), exact integers
        order      the stable ascending argsort of `score` (:66)
        p6, p8     split(count4, count6, numel, K)
An empty batch is left out (the reference fails on one)."""
import math

import torch


def thresholds(v, lamda=1.0):
    m = v.max(dim=-1, keepdim=True)[0]
    return m * 448 / 6 / math.pow(2, 10) * lamda, m * 448 / 28 / math.pow(2, 6) * lamda


def split(count4, count6, numel, k):
    p4_ratio = torch.tensor(count4) / numel
    p6_ratio = torch.tensor(count6) / numel - p4_ratio
    p8_ratio = 1 - p4_ratio - p6_ratio
    p6 = math.ceil(k * p6_ratio / 128) * 128
    p8 = math.ceil(k * p8_ratio / 128) * 128
    p6 = max(0, min(p6, k))
    return p6, max(0, min(p8, k - p6))


def run(batches, lamda=1.0):
    kept = [x.reshape(-1, x.shape[-1]).float().cpu().abs() for x in batches]
    kept = [v for v in kept if v.shape[0]]
    k = kept[0].shape[1]
    means64 = [v.double().sum(dim=0) / v.shape[0] for v in kept]
    means = [m.float() for m in means64]
    score64, score, score_ref = means64[0], means[0], torch.mean(kept[0], dim=0).float()
    for v, m64, m in zip(kept[1:], means64[1:], means[1:]):
        score64, score, score_ref = torch.max(score64, m64), torch.max(score, m), torch.max(score_ref, torch.mean(v, dim=0).float())
    value = torch.cat(kept, dim=0)
    t4, t6 = thresholds(value, lamda)
    count4, count6, numel = int((value < t4).sum()), int((value < t6).sum()), value.numel()
    p6, p8 = split(count4, count6, numel, k)
    return dict(means=means, score64=score64, score=score, score_ref=score_ref, count4=count4, count6=count6, numel=numel,
                order=torch.sort(score, stable=True).indices, p6=p6, p8=p8)
