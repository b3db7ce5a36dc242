"""Host-side callers of the forward: chunker, feature-file dataset, the evaluation loop and its
multi-GPU sharding.  Counterparts of
  * `process_split` / `pad`                       /root/reference/data/tools.py:81-86,100-114
  * `UCF_Dataset` / `XD_Dataset` / `Shang_Dataset` /root/reference/data/dataset.py:8-127 (test mode)
  * `test()`                                      /root/reference/test.py:46-212,
                                                   train/ucf_test.py:16-216, train/xd_test.py:15-210
  * `compute_ano_auc`                             /root/reference/test.py:332-348
  * `run_test` (robustness sweep)                 /root/reference/test2.py:35-123 (`PerturbationSweep`)
The model is any callable with the reference's `model(img, ev, padding_mask, text, lengths)` contract.
"""
from __future__ import annotations

import concurrent.futures
import contextlib
import csv
import math
import os
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

# per-dataset class keys of the reference's class-wise tables (/root/reference/test.py:20-43)
CLASS_KEYS = {
    'ucfcrime': ['Abuse', 'Arrest', 'Arson', 'Assault', 'Burglary', 'Explosion', 'Fighting', 'RoadAccidents',
                 'Robbery', 'Shooting', 'Shoplifting', 'Stealing', 'Vandalism', 'Normal'],
    'xd': ['normal', 'fighting', 'shooting', 'riot', 'abuse', 'car accident', 'explosion'],
    'shang': ['car', 'chasing', 'fall', 'fighting', 'monocycle', 'robbery', 'running', 'skateboard',
              'throwing_object', 'vehicle', 'vaudeville', 'normal'],
    'msad': ['Normal', 'Assault', 'Explosion', 'Fighting', 'Fire', 'Object_falling', 'People_falling', 'Robbery',
             'Shooting', 'Traffic_accident', 'Vandalism', 'Water_incident'],
}
# event-feature path rule: str.replace over the WHOLE path (dataset.py:36,67,112)
EVENT_DIR = {'ucfcrime': 'event_thr_10', 'xd': 'event_thr_10', 'msad': 'event_thr_10', 'shang': 'event'}


def host_cpu_share() -> int:
    """CPUs this process may actually use: min(affinity, cgroup quota).  A GPU box can expose hundreds of
    hardware threads while a one-GPU job is capped at a small quota; a torch intra-op pool sized to
    os.cpu_count() then oversubscribes it and every small host-side tensor op crawls."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return int(os.environ.get("IEFVAD_CPU_THREADS", n))


# ------------------------------------------------------------------------------------------------
# chunker + dataset
# ------------------------------------------------------------------------------------------------
def process_split(feat: np.ndarray, length: int) -> Tuple[np.ndarray, int]:
    """Test-time chunking (tools.py:100-114): len < length -> one zero-padded [length, D] block;
    otherwise len//length + 1 blocks [n, length, D], the last zero padded -- an ALL-zero block when
    len % length == 0.  dtype is preserved."""
    n = int(feat.shape[0])
    if n < length:
        out = np.zeros((length, feat.shape[1]), dtype=feat.dtype)
        out[:n] = feat
        return out, n
    nchunk = n // length + 1
    out = np.zeros((nchunk * length, feat.shape[1]), dtype=feat.dtype)
    out[:n] = feat
    return out.reshape(nchunk, length, feat.shape[1]), n


class VideoFeatureDataset(torch.utils.data.Dataset):
    """Test-mode dataset over a `path,label` CSV of image-feature .npy files; the event file is found
    with the reference's replace rule.  Items match the reference's:
    (img [n,T,D] or [T,D], ev, label, length)."""

    def __init__(self, clip_dim: int, file_path: str, dataset: str = 'ucfcrime'):
        with open(file_path, newline='') as f:
            rows = list(csv.DictReader(f))
        self.paths = [r['path'] for r in rows]
        self.labels = [r['label'] for r in rows]
        self.clip_dim = clip_dim
        self.event_dir = EVENT_DIR[dataset]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        p = self.paths[index]
        img = np.load(p)
        ev = np.load(p.replace('rgb', self.event_dir))
        img, n = process_split(img, self.clip_dim)
        ev, _ = process_split(ev, self.clip_dim)
        return torch.tensor(img), torch.tensor(ev), self.labels[index], n


def get_test_loader(args, dataset: Optional[str] = None):
    """`DataLoader(test_dataset, batch_size=1, shuffle=False)` (data/__getter__.py:27,39-40,66)."""
    ds = VideoFeatureDataset(args.visual_length, args.test_list, dataset or args.dataset)
    return torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False)


# ------------------------------------------------------------------------------------------------
# the training loader (data/tools.py:65-97, the test_mode == False branch of data/dataset.py, data/__getter__.py:5-84)
# ------------------------------------------------------------------------------------------------
NORMAL_LABEL = {'ucfcrime': 'Normal', 'msad': 'Normal', 'shang': 'normal'}        # dataset.py:24,28,100,104; xd has no filter


def segment_bounds(n: int, length: int = 256) -> np.ndarray:
    """`np.linspace(0, n, length + 1, dtype=np.int32)` of uniform_extract (tools.py:67) in integers: (i n) >> 8 for length = 256
    (n / 256 and i (n / 256) are exact in fp64, so linspace truncates exactly these values)."""
    if length & (length - 1):
        raise ValueError(f"segment_bounds: the integer identity holds for a power-of-two window, not for {length}")
    i = np.arange(length + 1, dtype=np.int64)
    return (i * int(n)) // length


def process_feat(feat: np.ndarray, length: int) -> Tuple[np.ndarray, int]:
    """Train-time window (tools.py:89-97 with is_random False, which is all the reference ever selects): n <= length rows ->
    the rows, zero padded, clip length n; more -> `length` segments (`segment_bounds`), each replaced by np.mean of its rows,
    clip length `length`.  Always fp32 (the reference hands back a short fp16 file as fp16; widening is exact).

    np.mean over axis 0 is an fp32 accumulator starting at +0, one add per row in ascending order, one division by the count,
    and for an fp16 file a rounding of the quotient to fp16.  Restated here over all segments at once: the j-th row of every
    segment is added in one vector operation, n // length (+ 1) of them instead of `length` np.mean calls -- the same adds in the
    same order per output element, so the same bits, and the host model of csrc/resample.h."""
    n, D = int(feat.shape[0]), int(feat.shape[1])
    out = np.zeros((length, D), dtype=np.float32)
    if n <= length:
        out[:n] = feat
        return out, n
    r = segment_bounds(n, length)
    start, count = r[:-1], r[1:] - r[:-1]
    with np.errstate(invalid='ignore', over='ignore'):      # non-finite values pass through as the arithmetic has it
        for j in range(int(count.max())):
            if j < int(count.min()):
                out += feat[start + j]                      # fp16 rows are widened by the fp32 destination of the add
            else:
                sel = np.nonzero(count > j)[0]
                out[sel] += feat[start[sel] + j]
        out /= count.astype(np.float32)[:, None]
        if feat.dtype == np.float16:
            out = out.astype(np.float16).astype(np.float32)
    return out, length


class TrainFeatureDataset(torch.utils.data.Dataset):
    """Train-mode counterpart of UCF_Dataset / XD_Dataset / Shang_Dataset over a `path,label` CSV.  `normal` True keeps the rows
    whose label is the dataset's normal label ('Normal'; 'normal' for shang), False the others, in file order (the reference's
    `.loc[...]` + `reset_index`); None keeps the whole list, which is also what 'xd' always does (XD_Dataset has no filter).
    Items are the reference's: (img [clip_dim, D] fp32, ev [clip_dim, D] fp32, label, clip length of the IMAGE file); the event
    file is resampled by its own row count."""

    def __init__(self, clip_dim: int, file_path: str, dataset: str = 'ucfcrime', normal: Optional[bool] = None):
        if dataset not in EVENT_DIR:
            raise ValueError('Dataset not supported')
        with open(file_path, newline='') as f:
            rows = list(csv.DictReader(f))
        if dataset != 'xd' and normal is not None:
            key = NORMAL_LABEL[dataset]
            rows = [r for r in rows if (r['label'] == key) == bool(normal)]
        self.paths = [r['path'] for r in rows]
        self.labels = [r['label'] for r in rows]
        self.clip_dim = clip_dim
        self.dataset = dataset
        self.normal = normal
        self.event_dir = EVENT_DIR[dataset]

    def __len__(self):
        return len(self.paths)

    def event_path(self, index: int) -> str:
        return self.paths[index].replace('rgb', self.event_dir)

    def load_raw(self, index: int) -> Tuple[np.ndarray, np.ndarray]:
        """The two feature files of an item as stored, [n_img, D] and [n_ev, D]."""
        return np.load(self.paths[index]), np.load(self.event_path(index))

    def __getitem__(self, index):
        img, ev = self.load_raw(index)
        img, n = process_feat(img, self.clip_dim)
        ev, _ = process_feat(ev, self.clip_dim)
        return torch.from_numpy(img), torch.from_numpy(ev), self.labels[index], n


def get_train_loaders(args, dataset: Optional[str] = None):
    """The train side of `get_loader` (data/__getter__.py): (normal_loader, abnormal_loader), both `shuffle=True, drop_last=True`,
    for ucfcrime / shang / msad; ONE loader with `shuffle=True` for xd.  batch_size = args.batch_size."""
    dataset = dataset or args.dataset
    if dataset not in EVENT_DIR:
        raise ValueError('Dataset not supported')
    if dataset == 'xd':
        ds = TrainFeatureDataset(args.visual_length, args.train_list, 'xd')
        return torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True)
    sets = [TrainFeatureDataset(args.visual_length, args.train_list, dataset, normal=flag) for flag in (True, False)]
    return tuple(torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, drop_last=True) for ds in sets)


# ------------------------------------------------------------------------------------------------
# metrics (sklearn, exactly the calls the reference makes)
# ------------------------------------------------------------------------------------------------
def compute_ano_auc(classwise_gt, classwise_roc, repeat_factor=16, normal_keys=('Normal',)):
    """test.py:332-348.  `normal_keys` covers the three variants of the filter: ('Normal',) in test.py:336,
    ('Normal', 'normal') in ucf_test.py:340, ('normal',) in xd_test.py:334."""
    from sklearn.metrics import roc_auc_score
    gt_abnormal, pred_abnormal = [], []
    for key in classwise_gt.keys():
        if key not in normal_keys and len(classwise_gt[key]) > 0:
            gt_abnormal.extend(np.concatenate(classwise_gt[key]).tolist())
            pred_abnormal.extend(np.concatenate(classwise_roc[key]).tolist())
    gt_abnormal = np.array(gt_abnormal)
    pred_abnormal = np.array(pred_abnormal)
    if len(np.unique(gt_abnormal)) > 1:
        return roc_auc_score(gt_abnormal, np.repeat(pred_abnormal, repeat_factor))
    return float('nan')


def evaluate_scores(scores: Sequence[np.ndarray], classes: Sequence[str], gt: np.ndarray, dataset: str,
                    verbose: bool = True, normal_keys=('Normal',), total_samples: bool = False,
                    log: Optional[Callable] = None) -> Dict[str, object]:
    """Metric tail of test() (test.py:155-175): ROC-AUC / AP on the x16-repeated snippet scores, Ano-AUC
    over the abnormal classes, per-class AUC/AP.  `scores` are per-video vectors in test-list order; gt
    is indexed by the running snippet offset (test.py:129,153)."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    keys = CLASS_KEYS[dataset]
    cw_pred = {k: [] for k in keys}
    cw_gt = {k: [] for k in keys}
    st = 0
    for s, c in zip(scores, classes):
        cw_pred[c].append(np.asarray(s))
        cw_gt[c].append(gt[16 * st:16 * (st + len(s))])
        st += len(s)
    ap1 = np.concatenate([np.asarray(s) for s in scores]).tolist()
    roc = roc_auc_score(gt, np.repeat(ap1, 16))
    ap = average_precision_score(gt, np.repeat(ap1, 16))
    ano = compute_ano_auc(cw_gt, cw_pred, normal_keys=normal_keys)
    if verbose:
        print("AUC1: {:.2f}  AP1: {:.2f}".format(roc * 100, ap * 100))
        print("Ano-AUC: {:.2f}".format(ano * 100))
    if log is not None:      # ucf_test.py:158-162 / xd_test.py:155-159
        log({'test/AP1': ap, 'test/ROC1': roc, 'test/Ano-AUC': ano})
    per_class = {}
    for c in keys:
        cls_pred = np.concatenate(cw_pred[c])   # raises on an empty class exactly as test.py:166-167 does
        cls_gt = np.concatenate(cw_gt[c])
        if len(cls_gt) == 0 or sum(cls_gt) == 0:
            continue
        c_roc = roc_auc_score(cls_gt, np.repeat(cls_pred, 16))
        c_ap = average_precision_score(cls_gt, np.repeat(cls_pred, 16))
        if verbose and total_samples:      # ucf_test.py:173-174
            print(c, 'ROC: {:.2f}  AP: {:.2f}'.format(c_roc * 100, c_ap * 100), end='\t')
            print(f"Total Samples: {len(cls_gt)}")
        elif verbose:
            print(c, 'ROC: {:.2f}  AP: {:.2f}'.format(c_roc * 100, c_ap * 100))
        if log is not None:                # ucf_test.py:175-178 / xd_test.py:170-173
            log({'classwise/ROC/' + c: c_roc, 'classwise/AP/' + c: c_ap})
        per_class[c] = (c_roc, c_ap)
    if verbose:
        print('-------------------------------------------------')
    return {"roc": roc, "ap": ap, "ano_auc": ano, "per_class": per_class}


def device_auc_ap(scores: torch.Tensor, gt: torch.Tensor, repeat: int = 16) -> Tuple[float, float]:
    """ROC-AUC and average precision of `np.repeat(scores, repeat)` against frame-level `gt` -- the metric tail of
    test.py:158-159, which costs sklearn a sort of 16 x N points on the host -- by the library's `iefvad_auc_ap`
    (csrc/metrics.h: one radix sort of (score, positive frames of the snippet) pairs, a scan, a reduction over the tie
    groups; the repeat is never materialised).  Ties as sklearn: thresholds are the DISTINCT score values.
    `scores` [N] on a HIP device; `gt` [N * repeat] (any dtype, non-zero = anomalous; host or device)."""
    from . import lib as _lib
    import ctypes as C
    if not scores.is_cuda:
        raise RuntimeError("device_auc_ap runs on a HIP device only (iefvad_auc_ap); on the host use evaluate_scores (sklearn)")
    s = scores.reshape(-1).to(torch.float32).contiguous()
    g = torch.as_tensor(gt).reshape(-1)
    if g.numel() != s.numel() * repeat:
        raise ValueError("gt must hold `repeat` frames per snippet")
    # the kernel counts every non-zero byte as an anomalous frame: one-byte ground truth (uint8 / bool) goes in as it is
    g = g if g.dtype in (torch.uint8, torch.bool) else (g != 0).to(torch.uint8)
    g = g.to(s.device, non_blocking=True).contiguous()
    lib = _lib.load_library()
    n = s.numel()
    with torch.cuda.device(s.device):
        ws = torch.empty(lib.iefvad_auc_ap_workspace_bytes(n) + 256, dtype=torch.uint8, device=s.device)
        off = (-ws.data_ptr()) % 256
        out = torch.empty(2, dtype=torch.float64, device=s.device)
        rc = lib.iefvad_auc_ap(C.c_void_p(s.data_ptr()), C.c_void_p(g.data_ptr()), n, repeat, C.c_void_p(out.data_ptr()),
                               C.c_void_p(out.data_ptr() + 8), C.c_void_p(ws.data_ptr() + off), ws.numel() - off,
                               C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("iefvad_auc_ap: " + _lib.last_error())
    auc, ap = out.cpu().tolist()
    return auc, ap


def _metric_inputs(scores: torch.Tensor, gt, repeat: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 scores [N] and one-byte ground truth [N * repeat] on the scores' device, as the metric entries read them (a tensor that
    already has that form comes back as it is)."""
    s = scores.reshape(-1).to(torch.float32).contiguous()
    g = torch.as_tensor(gt).reshape(-1)
    if g.numel() != s.numel() * repeat:
        raise ValueError("gt must hold `repeat` frames per snippet")
    g = g if g.dtype in (torch.uint8, torch.bool) else (g != 0).to(torch.uint8)
    return s, g.to(s.device, non_blocking=True).contiguous()


def device_grouped_auc_ap(scores: torch.Tensor, gt: torch.Tensor, group: torch.Tensor, ngroups: int,
                          repeat: int = 16) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`device_auc_ap` for up to 64 disjoint groups of snippets in one pass (the library's `iefvad_auc_ap_grouped`): the per-class
    loops of test.py:165-174 with group = class, the Ano-AUC of test.py:161 with one group that leaves the normal videos out.
    `group` [N] bytes: a value in [0, ngroups) puts the snippet into that group, 255 into none.  Returns
    (auc [ngroups], ap [ngroups], frames [ngroups, 2] = {frames, positive frames} per group) as numpy arrays, in ONE read-back.
    An empty group gives NaN / NaN, one class only gives auc NaN (sklearn raises there), no positive frame gives ap 0."""
    from . import lib as _lib
    import ctypes as C
    if not scores.is_cuda:
        raise RuntimeError("device_grouped_auc_ap runs on a HIP device only (iefvad_auc_ap_grouped); on the host use evaluate_scores (sklearn)")
    s, g = _metric_inputs(scores, gt, repeat)
    grp = torch.as_tensor(group).reshape(-1)
    if grp.numel() != s.numel():
        raise ValueError("group must hold one byte per snippet")
    grp = grp.to(device=s.device, dtype=torch.uint8).contiguous()
    lib = _lib.load_library()
    n = s.numel()
    with torch.cuda.device(s.device):
        ws = torch.empty(lib.iefvad_auc_ap_grouped_workspace_bytes(n, ngroups) + 256, dtype=torch.uint8, device=s.device)
        off = (-ws.data_ptr()) % 256
        out = torch.empty(4 * max(ngroups, 1), dtype=torch.float64, device=s.device)      # auc | ap | frames (int64 bits)
        rc = lib.iefvad_auc_ap_grouped(C.c_void_p(s.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(grp.data_ptr()), n, repeat, ngroups,
                                       C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8 * ngroups),
                                       C.c_void_p(out.data_ptr() + 16 * ngroups), C.c_void_p(ws.data_ptr() + off), ws.numel() - off,
                                       C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("iefvad_auc_ap_grouped: " + _lib.last_error())
    host = out.cpu().numpy()
    return host[:ngroups].copy(), host[ngroups:2 * ngroups].copy(), host[2 * ngroups:].view(np.int64).reshape(ngroups, 2).copy()


def evaluate_scores_device(scores, classes: Sequence[str], gt, dataset: str, verbose: bool = True, normal_keys=('Normal',),
                           total_samples: bool = False, log: Optional[Callable] = None) -> Dict[str, object]:
    """`evaluate_scores` with all three groups of sklearn calls replaced by library calls on ONE device-resident copy of the
    concatenated scores and of `gt`: `iefvad_auc_ap` for the global pair (test.py:158-159), one `iefvad_auc_ap_grouped` call with the
    class index of every snippet for the per-class pairs (test.py:165-174), one with a single group that leaves the `normal_keys`
    classes out for the Ano-AUC (test.py:161).  Same dict, same printed lines in the same order, same `log` calls.

    `scores`: per-video host vectors in test-list order (uploaded once), or `(tensor, lengths)` -- one device tensor of the
    concatenated scores plus the per-video lengths; then only the per-video class bytes go up and the results come back.  `gt` may be
    a host array or a device tensor.  The Ano-AUC is NaN where `compute_ano_auc` returns NaN; a class of `CLASS_KEYS[dataset]` without
    a video raises ValueError where the host function's `np.concatenate` does.  Where sklearn raises (a class whose frames are all
    positive, NaN scores) the value is NaN instead."""
    keys = CLASS_KEYS[dataset]
    if isinstance(scores, tuple) and len(scores) == 2 and torch.is_tensor(scores[0]):
        flat, lengths = scores[0].reshape(-1), [int(n) for n in scores[1]]
    else:
        lengths = [len(s) for s in scores]
        flat = torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.float32).reshape(-1) for s in scores]))
    if not flat.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("evaluate_scores_device runs on a HIP device only (iefvad_auc_ap, iefvad_auc_ap_grouped); "
                               "on the host use evaluate_scores (sklearn)")
        flat = flat.cuda()
    if len(lengths) != len(classes) or sum(lengths) != flat.numel():
        raise ValueError("one class and one length per video, the lengths adding up to the number of scores")
    index = {k: i for i, k in enumerate(keys)}
    cls_idx = np.array([index[c] for c in classes], dtype=np.uint8)          # KeyError for a class outside the table, as cw_pred[c] gives
    videos = np.bincount(cls_idx, minlength=len(keys))
    normal = np.array([k in normal_keys for k in keys])
    s, g = _metric_inputs(flat, gt, 16)
    # per-snippet group bytes from the per-video ones, expanded on the device: [class index | 0 = abnormal, 255 = left out]
    per_video = torch.from_numpy(np.stack([cls_idx, np.where(normal[cls_idx], 255, 0).astype(np.uint8)])).to(s.device)
    groups = torch.repeat_interleave(per_video, torch.tensor(lengths, device=s.device), dim=1, output_size=s.numel())
    roc, ap = device_auc_ap(s, g)
    c_roc, c_ap, c_frames = device_grouped_auc_ap(s, g, groups[0], len(keys))
    ano = float(device_grouped_auc_ap(s, g, groups[1], 1)[0][0])
    if verbose:
        print("AUC1: {:.2f}  AP1: {:.2f}".format(roc * 100, ap * 100))
        print("Ano-AUC: {:.2f}".format(ano * 100))
    if log is not None:
        log({'test/AP1': ap, 'test/ROC1': roc, 'test/Ano-AUC': ano})
    per_class = {}
    for i, c in enumerate(keys):
        if videos[i] == 0:
            raise ValueError("need at least one array to concatenate")      # np.concatenate([]) of test.py:166-167
        frames, positives = int(c_frames[i, 0]), int(c_frames[i, 1])
        if frames == 0 or positives == 0:
            continue
        r, a = float(c_roc[i]), float(c_ap[i])
        if verbose and total_samples:
            print(c, 'ROC: {:.2f}  AP: {:.2f}'.format(r * 100, a * 100), end='\t')
            print(f"Total Samples: {frames}")
        elif verbose:
            print(c, 'ROC: {:.2f}  AP: {:.2f}'.format(r * 100, a * 100))
        if log is not None:
            log({'classwise/ROC/' + c: r, 'classwise/AP/' + c: a})
        per_class[c] = (r, a)
    if verbose:
        print('-------------------------------------------------')
    return {"roc": roc, "ap": ap, "ano_auc": ano, "per_class": per_class}


SIMILARITY_KEYS = ("cos_i", "cos_e", "dist_i", "dist_e")


def similarity_rows(fused: torch.Tensor, image_mu: torch.Tensor, event_mu: torch.Tensor,
                    src_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The four per-snippet series of the reference's similarity plots (test.py:235-238, ucf_test.py:243-247) as ONE [4, nout] fp32
    tensor on the inputs' device, rows in `SIMILARITY_KEYS` order:
        F.cosine_similarity(fused, image_mu), F.cosine_similarity(fused, event_mu), torch.norm(fused - image_mu), torch.norm(fused - event_mu)
    over the last dimension.  The three tensors are [..., D] (leading dimensions are flattened); output row j reads flattened row
    `src_rows[j]` (every row in order without an index) -- the `[0:len]` slice of a padded batch is an index, not a copy.  On a HIP
    device one launch of the library's `iefvad_similarity_rows` (csrc/similarity.h; D = 768 or 512, fp32); on the CPU the four torch
    calls themselves."""
    D = int(fused.shape[-1])
    if image_mu.shape != fused.shape or event_mu.shape != fused.shape:
        raise ValueError("fused, image_mu and event_mu must have one shape")
    f, i, e = (t.reshape(-1, D) for t in (fused, image_mu, event_mu))
    if not f.is_cuda:
        if src_rows is not None:
            idx = torch.as_tensor(src_rows, dtype=torch.long, device=f.device)
            f, i, e = f[idx], i[idx], e[idx]
        f, i, e = f.float(), i.float(), e.float()
        return torch.stack([torch.nn.functional.cosine_similarity(f, i, dim=-1), torch.nn.functional.cosine_similarity(f, e, dim=-1),
                            torch.norm(f - i, dim=-1), torch.norm(f - e, dim=-1)])
    from . import lib as _lib
    import ctypes as C
    f, i, e = (t.to(torch.float32).contiguous() for t in (f, i, e))
    rows = int(f.shape[0])
    idx = None
    if src_rows is not None:
        idx = torch.as_tensor(src_rows).to(device=f.device, dtype=torch.int32).contiguous()
    nout = rows if idx is None else int(idx.numel())
    out = torch.empty(4, nout, dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device):
        rc = _lib.load_library().iefvad_similarity_rows(C.c_void_p(f.data_ptr()), C.c_void_p(i.data_ptr()), C.c_void_p(e.data_ptr()), rows, D,
                                                        C.c_void_p(idx.data_ptr() if idx is not None and nout else None), nout,
                                                        C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(f.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("iefvad_similarity_rows: " + _lib.last_error())
    return out


# ------------------------------------------------------------------------------------------------
# the evaluation loop
# ------------------------------------------------------------------------------------------------
def _has_nan(t: torch.Tensor) -> bool:
    """`torch.isnan(t).any()` (test.py:90,93) without a full boolean pass in the common case: a NaN element makes the sum
    NaN, so only a NaN sum (a real NaN, or +inf and -inf meeting) pays for the exact scan.  On the host this check was a
    third of the per-video loop's time."""
    if not t.is_floating_point():
        return False
    s = t.sum(dtype=torch.float32) if t.dtype in (torch.float16, torch.bfloat16) else t.sum()
    return bool(torch.isnan(s)) and bool(torch.isnan(t).any())


def online_windows(n: int, stride: int, history: int = 256) -> List[Tuple[int, int, int]]:
    """The trailing windows of a video of `n` snippets as `MMFMIL.forward_videos_online` evaluates them (csrc/window_plan.h): a list of
    (start, end, read0), one per window j = 1 .. ceil(n / stride) with end = min(j stride, n), start = max(0, end - history), read0 =
    (j - 1) stride.  Window j holds rows [start, end) of the video and zero rows behind them; only snippets [read0, end) are read out
    of it, rows read0 - start .. of the window.  1 <= stride <= history <= 256 (ValueError otherwise)."""
    from .model import online_params
    stride, history = online_params(stride, history)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"a video needs at least one snippet (got {n!r})")
    ends = [min(j * stride, int(n)) for j in range(1, (int(n) + stride - 1) // stride + 1)]
    return [(max(0, e - history), e, j * stride) for j, e in enumerate(ends)]


def video_chunks(n: int, T: int) -> int:
    # chunks of a video of n rows without the loader's all-zero chunk: the rule of `video_chunks` in csrc/iefvad.hip
    return n // T + (1 if n % T else 0) if n >= T else 1


def _item_class(item, dataset, label_map):
    """Class name of one DataLoader item (batch_size=1), remapped where the reference remaps it."""
    cls = item[2][0] if isinstance(item[2], (list, tuple)) else item[2]
    if label_map is not None and (dataset == 'xd' or isinstance(label_map, _AlwaysRemap)):
        cls = label_map[cls.split('-')[0]]            # xd_test.py:68 / test.py:80-81
    return cls


def _unpack_item(item, maxlen, dataset, label_map):
    """Shape rule of test.py:77-88 applied to one DataLoader item (batch_size=1)."""
    img = item[0].squeeze(0)
    ev = item[1].squeeze(0)
    cls = _item_class(item, dataset, label_map)
    length = int(item[3])
    if length < maxlen:
        img = img.unsqueeze(0)
        ev = ev.unsqueeze(0)
    if _has_nan(img):                                 # conditional nan_to_num, test.py:90-95
        img = torch.nan_to_num(img, nan=0.0)
    if _has_nan(ev):
        ev = torch.nan_to_num(ev, nan=0.0)
    return img, ev, cls, length


def _unpack_rows(item, maxlen, dataset, label_map):
    """One DataLoader item (batch_size=1, chunked and zero padded by the loader as the reference's is) reduced to what
    crosses the boundary in the ragged path: per modality the item's own [..., D] tensor, whose first `length` rows are the
    valid ones (no view is built: two tensor ops per video were a third of the loop's host time on short videos)."""
    cls = _item_class(item, dataset, label_map)
    length = int(item[3])
    img, ev = item[0], item[1]
    if not img.is_contiguous():
        img = img.contiguous()
    if not ev.is_contiguous():
        ev = ev.contiguous()
    return img, ev, cls, length


class _Stager:
    """`slots` reusable PINNED staging slots, taken in turn; a slot is reused only after the event behind its last copy has
    completed.  What is staged, and how a slot's buffers grow, is the subclass's."""

    def __init__(self, device, slots: int = 2, threads: int = 0):
        self.device = torch.device(device)
        self.threads = threads or max(1, min(8, host_cpu_share() // 2))      # host threads of one staging copy
        self.bufs = [[None, None] for _ in range(slots)]      # per slot: image / event pinned byte buffers
        self.events = [None] * slots
        self.turn = 0

    def _next_slot(self):
        slot = self.turn
        self.turn = (self.turn + 1) % len(self.bufs)
        if self.events[slot] is not None:
            self.events[slot].synchronize()
        return slot

    def _sent(self, slot):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.events[slot] = ev


class _PinnedStager(_Stager):
    """Host -> device hand-over of the evaluation loop.  The reference does `img.to(device)` on pageable tensors
    (test.py:90-95), a synchronous staged copy at a few GB/s that blocks the host for longer than a one-chunk forward
    takes on the device.  Here the chunks of a forward are gathered into one of two reusable PINNED buffers (one host
    memcpy, which also does the torch.cat of a packed batch) and sent with an asynchronous copy on the current stream."""

    def _buffer(self, slot, m, nbytes):
        b = self.bufs[slot][m]
        if b is None or b.numel() < nbytes:
            b = torch.empty(max(nbytes, 1 << 22), dtype=torch.uint8, pin_memory=True)
            self.bufs[slot][m] = b
        return b

    def upload(self, imgs, evs, dt):
        slot = self._next_slot()
        out = []
        for m, parts in enumerate((imgs, evs)):
            n = sum(int(p.shape[0]) for p in parts)
            shape = (n,) + tuple(parts[0].shape[1:])
            count = n * int(parts[0].shape[1]) * int(parts[0].shape[2])
            esize = torch.empty(0, dtype=dt).element_size()
            host = self._buffer(slot, m, count * esize)[:count * esize].view(dt).view(shape)
            off = 0
            for p in parts:
                host[off:off + p.shape[0]].copy_(p)          # casts when the batch was widened
                off += p.shape[0]
            out.append(host.to(self.device, non_blocking=True))
        self._sent(slot)
        return out[0], out[1]


class _RowStager(_Stager):
    """Host -> device hand-over of VALID rows (the packed evaluation loop through `MMFMIL.forward_videos`): the feature rows
    of a batch of videos are copied, without their zero padding, into one of `slots` reusable pinned buffers -- by a few
    threads when the batch is large -- and sent with one asynchronous copy per modality on the current stream.  Nothing on
    the host reads the rows: the NaN scan of test.py:90-95 happens on the device (csrc/ragged.h)."""

    def _buffer(self, slot, m, nbytes):
        b = self.bufs[slot][m]
        if b is None or b.numel() < nbytes:
            # pinning memory costs milliseconds per 100 MB: grow EVERY slot now (the first pass over a list is the warm-up,
            # later passes must not meet a slot that was never used at this size), with head room for uneven batches
            size = max(int(nbytes * 1.5), 1 << 22)
            for s_ in range(len(self.bufs)):
                for m_ in range(2):
                    old = self.bufs[s_][m_]
                    if old is None or old.numel() < size:
                        if self.events[s_] is not None:
                            self.events[s_].synchronize()
                        self.bufs[s_][m_] = torch.empty(size, dtype=torch.uint8, pin_memory=True)
            b = self.bufs[slot][m]
        return b

    def stage(self, imgs, evs, dt, lens=None):
        """Host half of `upload`: the rows of all videos into the next pinned slot.  Touches no stream (it only waits for the
        slot's previous copy), so a worker thread can run it while the caller's thread enqueues the previous batch.
        `lens` given: imgs / evs are contiguous [..., D] tensors whose FIRST lens[i] rows are taken."""
        slot = self._next_slot()
        D = int(imgs[0].shape[-1])
        if lens is None:
            lens = [int(p.shape[0]) for p in imgs]
        total = sum(lens)
        esize = torch.empty(0, dtype=dt).element_size()
        hosts = [self._buffer(slot, m, total * D * esize)[:total * D * esize].view(dt).view(total, D) for m in range(2)]
        if all(p.dtype == dt and p.is_contiguous() for parts in (imgs, evs) for p in parts):
            # one library call per modality: the rows of all videos gathered into the pinned buffer by a few host threads
            # (no GIL, no per-video tensor op: ~90 us of torch dispatch per video was 10x the forward's time on short videos)
            import ctypes as C
            from . import lib as _lib
            lib = _lib.load_library()
            n = len(lens)
            sizes = (C.c_size_t * n)(*[l * D * esize for l in lens])
            for host, parts in zip(hosts, (imgs, evs)):
                ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in parts])
                if lib.iefvad_host_gather(C.c_void_p(host.data_ptr()), ptrs, sizes, n, self.threads) != 0:
                    raise RuntimeError("iefvad_host_gather: " + _lib.last_error())
        else:                                                     # a widened (mixed-dtype) batch: torch casts while copying
            off = 0
            for i, l in enumerate(lens):
                hosts[0][off:off + l].copy_(imgs[i].reshape(-1, D)[:l])
                hosts[1][off:off + l].copy_(evs[i].reshape(-1, D)[:l])
                off += l
        return slot, hosts

    def send(self, staged):
        """Device half: one asynchronous copy per modality on the current stream.  Returns two [sum(len), D] device tensors."""
        slot, hosts = staged
        out = [h.to(self.device, non_blocking=True) for h in hosts]
        self._sent(slot)
        return out[0], out[1]

    def upload(self, imgs, evs, dt, lens=None):
        """imgs / evs: per video [len, D] host tensors (views are fine), or with `lens` contiguous [..., D] tensors of which the
        first lens[i] rows count.  Returns two [sum(len), D] device tensors."""
        return self.send(self.stage(imgs, evs, dt, lens))


class _ScoreSink:
    """What the forwards of one `score_loader` call leave behind.  Results stay on the model's device until the loop is over: the
    reference synchronises three times per video (`.cpu()` of prob / w_i / w_e, test.py:119-151); here the forwards are enqueued
    back to back and the scores of all videos come back in ONE device-to-host copy at the end (`finish`)."""

    def __init__(self):
        self.classes: List[str] = []
        self.dev_prob, self.dev_wi, self.dev_we = [], [], []      # per forward: flat fp32 device vectors
        self.spans: List[Tuple[int, int]] = []     # (offset into the concatenated device vectors, valid length) per video
        self.total = 0
        self.dev_sim: Optional[List[torch.Tensor]] = None     # score_loader(similarity=True): per forward [4, valid snippets of its videos]
        self.dev_rows: Optional[Dict[str, List[torch.Tensor]]] = None   # score_loader(row_outputs=...): per key, per forward [valid snippets, D]
        # score_loader(trajectory=True): per forward ([steps + 1, slots], [steps, slots]); score_loader(fusion_variants=): per forward ([V, slots],)
        self.dev_traj: Optional[List[Tuple[torch.Tensor, ...]]] = None

    def add(self, logits, wi, we, lens, stride=None, sim=None, rows=None, traj=None):
        """One forward's flat fp32 vectors over videos of `lens` snippets: back to back (the valid-row routes), or video i in
        stride[i] slots of which the first lens[i] count (the padded route: its chunks * maxlen).  `sim`: the forward's
        `similarity_rows` over the valid snippets of its videos, back to back.  `rows`: the forward's dict, from which the
        [valid snippets, D] tensors of `dev_rows` are kept (on the device, as they are)."""
        if sim is not None:
            self.dev_sim.append(sim)
        if self.dev_traj is not None and traj is not None:      # laid out like `logits`: the same slots, one row per step
            self.dev_traj.append(traj)
        if self.dev_rows is not None and rows is not None:
            for k, v in self.dev_rows.items():
                v.append(rows[k])
        self.dev_prob.append(logits)
        self.dev_wi.append(wi)
        self.dev_we.append(we)
        off = self.total
        for n, s in zip(lens, lens if stride is None else stride):
            self.spans.append((off, n))                      # logits1[0:len_cur] -> sigmoid, test.py:119-121
            off += s
        self.total = off

    def finish(self, device, return_device):
        """(scores, classes, w_i_mean, w_e_mean[, all scores as one device tensor][, similarity]): per-video views of three host
        vectors; with `dev_sim` a last result {key of SIMILARITY_KEYS: per-video views of that series}."""
        valid = sum(n for _, n in self.spans)
        simv = None
        if self.dev_prob:
            # ONE device-to-host copy for the three vectors (sigmoid once, on the device, on the concatenated logits)
            alld = torch.stack([torch.sigmoid(torch.cat(self.dev_prob)), torch.cat(self.dev_wi), torch.cat(self.dev_we)])
            if self.dev_sim is None:
                allv = alld.cpu().numpy()
            else:                                # ... and the four similarity series ride in the same copy
                flat = torch.cat([alld.reshape(-1), torch.cat(self.dev_sim, dim=1).reshape(-1)]).cpu().numpy()
                allv, simv = flat[:3 * self.total].reshape(3, self.total), flat[3 * self.total:].reshape(4, valid)
        else:
            alld = torch.zeros(3, 0, device=device)
            allv = np.zeros((3, 0), np.float32)
        scores, wi_means, we_means = ([v[o:o + n] for o, n in self.spans] for v in allv)
        res = (scores, self.classes, wi_means, we_means)
        if return_device:
            packed = valid == self.total      # no gaps: the valid snippets already lie back to back
            res += (alld[0] if packed else torch.cat([alld[0, o:o + n] for o, n in self.spans]),)
        if self.dev_sim is not None:
            if simv is None:
                simv = np.zeros((4, 0), np.float32)
            offs = np.concatenate([[0], np.cumsum([n for _, n in self.spans])]).astype(np.int64)
            res += ({k: [v[offs[i]:offs[i + 1]] for i in range(len(self.spans))] for k, v in zip(SIMILARITY_KEYS, simv)},)
        return res


def _batch_dtype(pend):
    """(dtype in which a batch of (img, ev, ...) entries is staged, whether that widens any of them).  The dtype is the files'
    (dataset.py:37-38,49-50); the model widens with `.to(torch.float)` per modality (imf_vad.py:41-42), so a batch that mixes
    dtypes -- across videos OR between the two modalities -- is widened to fp32 rather than narrowed to the first tensor's type."""
    dts = {p[0].dtype for p in pend} | {p[1].dtype for p in pend}
    return (torch.float32, True) if len(dts) > 1 else (pend[0][0].dtype, False)


def _lane_stream(stream):
    """Where a lane's copies and forwards are enqueued: on its own HIP stream, with one lane on the current stream."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _score_padded(models, stagers, streams, loader, sink, maxlen, device, dataset, label_map, batch_chunks, skip_empty_chunks,
                  similarity=False, trajectory=False, variants=(), samples=None):
    """Padded route (the only one on the CPU): `model(img, ev, ...)` on zero-padded chunks, one forward per video
    (batch_chunks <= 0) or per batch, which closes as soon as it holds `batch_chunks` chunks; forwards round-robin over the lanes.
    `_unpack_item` has applied the NaN rule in each tensor's own dtype; a mixed batch is widened while it is staged.
    `similarity`: each forward's `fused` / `image_mu` / `event_mu` are reduced to the four series of `similarity_rows` before the next
    forward overwrites them; the index is the `[0:len]` slice of every video of the batch (test.py:142)."""
    def forward(pend, k):
        dt, _ = _batch_dtype(pend)
        with _lane_stream(streams[k]):
            if stagers[k] is not None:
                img, ev = stagers[k].upload([p[0] for p in pend], [p[1] for p in pend], dt)
            else:
                img = torch.cat([p[0].to(dt) for p in pend], dim=0).to(device)
                ev = torch.cat([p[1].to(dt) for p in pend], dim=0).to(device)
            if samples is not None:      # snippet ids: the snippet's index among the valid snippets of the whole list (0 on pad rows)
                ids = torch.zeros(sum(p[0].shape[0] for p in pend) * maxlen, dtype=torch.int32)
                slot = 0
                for ci, _, n in pend:
                    ids[slot:slot + n] = torch.arange(seen[0], seen[0] + n, dtype=torch.int32)
                    slot, seen[0] = slot + ci.shape[0] * maxlen, seen[0] + n
                out = models[k].forward_samples(img, ev, samples[0], samples[1], scale=samples[2], sample_rows=ids.to(device))
            else:
                out = models[k](img, ev, None, None, None, **(dict(trajectory=True) if trajectory else dict(fusion_variants=variants) if variants else {}))
            logits = out['logits'].reshape(-1)
            traj = None
            if samples is not None:
                traj = (out['logits_samples'].reshape(samples[0], -1), torch.stack([out['score_mean'].reshape(-1), out['score_std'].reshape(-1)]))
            if trajectory:
                ls = out['logits_steps']
                traj = (ls.reshape(ls.shape[0], -1), out['delta_norm'].reshape(ls.shape[0] - 1, -1))
            if variants:
                traj = (out['logits_variants'].reshape(len(variants), -1),)
            if 'w_i_mean' in out:
                wi, we = out['w_i_mean'].reshape(-1), out['w_e_mean'].reshape(-1)
            else:
                wi = out['w_i'].reshape(-1, out['w_i'].shape[-1]).mean(dim=-1)     # test.py:131-136
                we = out['w_e'].reshape(-1, out['w_e'].shape[-1]).mean(dim=-1)
            lens, stride = [n for _, _, n in pend], [ci.shape[0] * maxlen for ci, _, _ in pend]
            sim = None
            if similarity:
                if any(k not in out for k in ('fused', 'image_mu', 'event_mu')):
                    raise ValueError(_NEEDS_FULL)
                starts = np.concatenate([[0], np.cumsum(stride)[:-1]])
                index = np.concatenate([np.arange(o, o + n, dtype=np.int32) for o, n in zip(starts, lens)])
                sim = similarity_rows(out['fused'], out['image_mu'], out['event_mu'], torch.from_numpy(index))
            sink.add(logits.float(), wi.float(), we.float(), lens, stride, sim, traj=traj)

    seen = [0]      # valid snippets of the videos already sent
    pend, pend_chunks, nsent = [], 0, 0
    for item in loader:
        img, ev, cls, n = _unpack_item(item, maxlen, dataset, label_map)
        sink.classes.append(cls)
        if batch_chunks > 0 and skip_empty_chunks and n >= maxlen and n % maxlen == 0:
            img, ev = img[:-1], ev[:-1]               # the all-zero chunk (tools.py:105-112)
        pend.append((img, ev, n))
        pend_chunks += img.shape[0]
        if batch_chunks <= 0 or pend_chunks >= batch_chunks:
            forward(pend, nsent % len(models))
            pend, pend_chunks, nsent = [], 0, nsent + 1
    if pend:
        forward(pend, nsent % len(models))


_NEEDS_FULL = ('similarity=True reads the forward\'s fused, image_mu and event_mu: build the model with outputs="full" '
               '(outputs="scores" / "weights" do not return them)')


def _score_rows_loop(models, stagers, streams, loader, sink, maxlen, dataset, label_map, batch_chunks, similarity=False, row_outputs=(),
                     attn_layers=(), trajectory=False, variants=(), samples=None, online=None):
    """Valid-row loop around `MMFMIL.forward_videos` (`online=(stride, history)`: around `MMFMIL.forward_videos_online`): a batch closes as soon as its videos make up `batch_chunks` chunks; batches go
    round-robin over the lanes.  The staging copy of batch k + 1 (host threads inside the library, no GIL) runs on a worker thread
    while this thread sends batch k and enqueues its forward; batches complete in order.
    `similarity`: every forward also returns its [4, n] block of series (`forward_videos(similarity=True)`) for the sink.
    `row_outputs`: every forward also returns those [n, D] tensors (`forward_videos(outputs=...)`); the sink keeps them on the device.
    `attn_layers`: every forward also returns the attention maps of those layers (`forward_videos(attn_maps=...)`), kept the same way."""
    def stage(pend, k):
        dt, widened = _batch_dtype(pend)
        if widened:               # a narrower video is widened at staging: its own dtype's inf -> max rule applies first (test.py:90-95)
            pend = [tuple(torch.nan_to_num(t, nan=0.0) if (t.dtype != dt and _has_nan(t)) else t for t in (p[0], p[1])) + (p[2],)
                    for p in pend]
        lens = [n for _, _, n in pend]
        return k, stage_pool.submit(stagers[k].stage, [p[0] for p in pend], [p[1] for p in pend], dt, lens), lens

    def send_and_forward(k, fut, lens):
        staged = fut.result()
        with _lane_stream(streams[k]):
            img, ev = stagers[k].send(staged)
            if samples is not None:      # snippet ids: the snippet's index among the valid snippets of the whole list
                ids = torch.arange(seen[0], seen[0] + sum(lens), dtype=torch.int32, device=img.device)
                seen[0] += sum(lens)
                out = models[k].forward_videos_samples(img, ev, lens, samples[0], samples[1], scale=samples[2], nan_to_num=True, sample_rows=ids)
            elif online is not None:
                out = models[k].forward_videos_online(img, ev, lens, online[0], history=online[1], nan_to_num=True)
            else:
                out = models[k].forward_videos(img, ev, lens, nan_to_num=True, **sim_kw)
        sink.add(out['logits'], out['w_i_mean'], out['w_e_mean'], lens, sim=out.get('similarity'), rows=out,
                 traj=(out['logits_steps'], out['delta_norm']) if trajectory else (out['logits_variants'],) if variants else
                 (out['logits_samples'], torch.stack([out['score_mean'], out['score_std']])) if samples is not None else None)

    sim_kw = dict(similarity=True) if similarity else dict(outputs=row_outputs) if row_outputs else \
        dict(attn_maps=attn_layers) if attn_layers else dict(trajectory=True) if trajectory else \
        dict(fusion_variants=variants) if variants else {}

    seen = [0]      # valid snippets of the batches already sent (batches complete in order)
    stage_pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    inflight = []                                   # batches handed to the worker and not sent yet: ONE after every turn of the loop
    pend, pend_chunks, nstaged = [], 0, 0
    try:
        for item in loader:
            img, ev, cls, n = _unpack_rows(item, maxlen, dataset, label_map)
            sink.classes.append(cls)
            pend.append((img, ev, n))
            pend_chunks += video_chunks(n, maxlen)
            if pend_chunks >= batch_chunks:
                inflight.append(stage(pend, nstaged % len(models)))
                pend, pend_chunks, nstaged = [], 0, nstaged + 1
                if len(inflight) > 1:
                    send_and_forward(*inflight.pop(0))
        if pend:
            inflight.append(stage(pend, nstaged % len(models)))
        for batch in inflight:
            send_and_forward(*batch)
    finally:
        stage_pool.shutdown(wait=True)              # also when a forward raised: the worker thread must not outlive the call


def _score_rows_list(model, loader, sink, maxlen, dataset, label_map, batch_chunks, host_list_bytes, wire_bf16, similarity=False,
                     row_outputs=()):
    """Valid-row route with the walk inside the library (`MMFMIL.forward_videos_host`, csrc/hostpipe.h): this thread only collects
    each video's host tensor and length; one library call per `host_list_bytes` of features stages, sends and scores them pass by
    pass.  Same batches, same kernels as `_score_rows_loop` (which remains for models without the entry, lanes > 1 callers that
    ask for it with host_list=False, and device-resident loaders)."""
    def forward(group):
        wire = torch.bfloat16 if (wire_bf16 and group[0][0].dtype == torch.float32) else None
        lens = [g[2] for g in group]
        out = model.forward_videos_host([g[0] for g in group], [g[1] for g in group], lens, nan_to_num=True,
                                        batch_chunks=batch_chunks, wire_dtype=wire, **sim_kw)
        sink.add(out['logits'], out['w_i_mean'], out['w_e_mean'], lens, sim=out.get('similarity'), rows=out)

    sim_kw = dict(similarity=True) if similarity else dict(outputs=row_outputs) if row_outputs else {}

    group, gbytes = [], 0
    for item in loader:
        img, ev, cls, n = _unpack_rows(item, maxlen, dataset, label_map)
        sink.classes.append(cls)
        if img.is_cuda or ev.is_cuda:
            raise ValueError("host_list=True expects the loader's tensors in host memory")
        if img.dtype != ev.dtype or img.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            # the model widens both with `.to(torch.float)` (imf_vad.py:41-42); the NaN rule applies in the file's own dtype first
            img, ev = (torch.nan_to_num(t, nan=0.0) if _has_nan(t) else t for t in (img, ev))
            img, ev = img.float(), ev.float()
        if group and group[0][0].dtype != img.dtype:
            forward(group)                                    # a library call takes one feature dtype
            group, gbytes = [], 0
        group.append((img, ev, n))
        gbytes += 2 * n * img.shape[-1] * img.element_size()
        if gbytes >= host_list_bytes:
            forward(group)
            group, gbytes = [], 0
    if group:
        forward(group)


def score_loader(model: Callable, test_loader: Iterable, maxlen: int, device, dataset: str = 'ucfcrime',
                 label_map=None, batch_chunks: int = 0, skip_empty_chunks: bool = True, lanes: int = 1,
                 ragged: Optional[bool] = None, host_list: bool = True, host_list_bytes: int = 1 << 30, wire_bf16: bool = False,
                 return_device: bool = False, similarity=False, row_outputs=None, attn_maps=None, steps: Optional[int] = None,
                 trajectory: bool = False, fusion_variants=None, score_samples: Optional[int] = None, sample_seed: Optional[int] = None,
                 sample_scale: float = 1.0, online_stride: Optional[int] = None, online_history: int = 256):
    """Per-video sigmoid scores and mean fusion weights, in loader order.

    batch_chunks == 0: one forward per video with B = that video's chunk count -- the reference's call
    pattern (test.py:76-117).  batch_chunks > 0: chunks of consecutive videos are packed into one
    forward of up to `batch_chunks` chunks; legal because chunks are independent batch rows
    (imf_vad.py:115 attends within a chunk), and the trailing all-zero chunk of a len % 256 == 0 video,
    whose rows the reference slices away (test.py:121), is not computed when `skip_empty_chunks`.

    `ragged` (default: whenever the model has `forward_videos`, i.e. `iefvad_amd.MMFMIL` on a HIP device, and batch_chunks > 0):
    the packed batches go through `MMFMIL.forward_videos` -- only the VALID rows of every video are staged and uploaded, the
    chunker, the conditional nan_to_num (test.py:90-95) and the `[0:len]` slicing run on the device, and no stage computes the
    padding (one pad row per chunk stands for all of them, csrc/ragged.h).  Same scores (bit for bit in the f32 and bf16 modes).

    `host_list` (default; ragged mode with host-resident loader tensors): the walk over the list happens inside the library
    (`iefvad_forward_videos_host`): Python hands over each video's tensor and length, the library packs, stages, sends and scores
    pass by pass with its own worker thread and copy stream -- one call per `host_list_bytes` of features.  `lanes` is not used then.
    `wire_bf16` (list path, fp32 features, a compute="bf16" model): the rows are rounded to bf16 while they are staged and half the
    bytes cross PCIe (`MMFMIL.forward_videos_host(wire_dtype=torch.bfloat16)`); off by default.

    lanes > 1 (HIP devices, `iefvad_amd.MMFMIL`): consecutive forwards go round-robin to `lanes` HIP streams, each with a
    lane of the model (`MMFMIL.lanes`: same parameters, own library handle and workspace) and its own pinned staging.
    Same kernels on the same inputs, so every score is bit-identical to lanes = 1; what changes is that the one- and
    two-chunk forwards of the per-video pattern, each of which fills a fraction of the chip, overlap.

    `return_device`: a fifth result, the scores of all videos as ONE tensor on the model's device (valid snippets in loader order --
    what `evaluate_scores_device` takes together with the per-video lengths), so a device metric tail needs no upload.

    `similarity`: a last result, {"cos_i", "cos_e", "dist_i", "dist_e"} -> per-video arrays: cosine similarity and Euclidean distance of
    every snippet's `fused` row to its `image_mu` / `event_mu` rows (`similarity_rows`; the series of test.py:235-238).  The padded route
    is taken with the caller's `batch_chunks` -- in f32 and bf16 both routes give the same bits, so the scores do not move (the valid-row
    routes: `similarity="rows"` and `row_outputs` below) -- and the model must return the full dict (`outputs="full"`).  The series stay on the device
    and come back with the scores' one copy.
    `similarity="rows"` (opt-in): the same last result from the valid-row routes -- the host-list walk, or the `forward_videos` loop
    (`host_list=False`, `lanes > 1` included): every library call reduces the series of its valid rows from the pass's own fused / mu
    rows (`MMFMIL.forward_videos(similarity=True)`, csrc/similarity.h), no padding is computed and the model may be built with any
    `outputs=`.  Needs a HIP device, a model with `forward_videos` and batch_chunks > 0 (ValueError otherwise).  In f32 and bf16 the
    series are the bits of `similarity=True`.

    `row_outputs` ("full", or names from `iefvad_amd.OUTPUT_KEYS`; opt-in): the valid-row routes -- the host-list walk, or the
    `forward_videos` loop -- with `outputs=row_outputs` on every library call (`iefvad_forward_videos_full` / `_host_full`): the
    [rows, D] tensors of the reference's dict for the VALID snippets only, whatever `outputs=` the model was built with.  The returned
    tuple does not change; `score_loader.last_result` becomes {"row_outputs": {name: ONE [N, D] fp32 device tensor, the videos in
    list order}, "row_offsets": int64 array of len(videos) + 1 offsets into N}.  Nothing D-wide is copied to the host here.  Needs what
    `similarity="rows"` needs; it does not combine with `similarity` (ValueError).

    `attn_maps` (True, or an iterable of encoder layer indices; opt-in): the `forward_videos` loop with `attn_maps=` on every call
    (`iefvad_forward_videos_attn`, csrc/attention_maps.h).  The returned tuple and the scores do not change; `score_loader.last_result`
    becomes {"attn_maps": {"image", "event": ONE [n, N, T] fp32 device tensor each -- the head-averaged attention weights of the N
    valid snippets over the T keys of their chunks, layers in the order of "layers"; "layers": the n layer indices, ascending;
    "row_offsets": int64 array of len(videos) + 1 offsets into N}}.  ValueError with ragged=False, a CPU device, `row_outputs` or
    `similarity`.

    `steps` (an integer in 0 .. K; a model with `set_steps`, i.e. `iefvad_amd.MMFMIL`): the walk runs with only the first `steps`
    refinement blocks (`MMFMIL.set_steps`); the model's own count is restored afterwards, also when a forward raises.
    `trajectory=True` (the per-video / padded route and the `forward_videos` loop; HIP device): every forward also returns its
    refinement trajectory (`forward(..., trajectory=True)` / `forward_videos(..., trajectory=True)`).  The returned tuple does not
    change; `score_loader.last_result` becomes {"trajectory": {"scores_steps": [steps + 1, N] float32 array, the sigmoid of the logits
    after 0 .. steps steps for the N valid snippets, the videos in list order; "delta_norm": [steps, N] array of ||z_{k+1} - z_k||;
    "scores_steps_device": the first one as a device tensor; "row_offsets": int64 array of len(videos) + 1 offsets into N}}.  The
    host-list walk does not take it: on the valid-row routes pass host_list=False (ValueError otherwise); it does not combine with
    `similarity`, `row_outputs` or `attn_maps`.
    `fusion_variants` (True: all four, or names from "fused", "image", "event", "equal"; the per-video / padded route and the
    `forward_videos` loop; HIP device): every forward also returns its fusion ablations (`forward(..., fusion_variants=...)` /
    `forward_videos(..., fusion_variants=...)`).  The returned tuple does not change; `score_loader.last_result` becomes {"variants":
    {"names": the names in the order asked for; "scores": per video a [V, snippets] float32 array, the sigmoid of the variants' logits;
    "scores_device": ONE [V, N] device tensor of the N valid snippets, the videos in list order; "row_offsets": int64 array of
    len(videos) + 1 offsets into N}}.  The host-list walk does not take it: on the valid-row routes pass host_list=False (ValueError
    otherwise); it does not combine with `trajectory`, `similarity`, `row_outputs` or `attn_maps`.
    `score_samples=S` with `sample_seed=` (and `sample_scale=`, default 1; the per-video / padded route and the `forward_videos` loop; HIP
    device): every forward is `MMFMIL.forward_samples` / `forward_videos_samples` -- S Monte Carlo draws of every snippet's score from the
    heads' own Gaussians (this package's own semantics; the reference never samples).  The snippet id of a draw is the snippet's index
    among the valid snippets of the whole list, so a snippet's samples do not depend on the route or on `batch_chunks`.  The returned
    tuple does not change; `score_loader.last_result` becomes {"samples": {"scores_mean", "scores_std": per video a [snippets] float32
    array, mean and population standard deviation of the S scores, formed on the device; "logits_samples_device": ONE [S, N] device
    tensor of the N valid snippets, the videos in list order (apply the sigmoid); "row_offsets": int64 array of len(videos) + 1 offsets
    into N}}.  The host-list walk does not take it: on the valid-row routes pass host_list=False (ValueError otherwise); it combines
    with none of the other extras (`steps`, `trajectory`, `fusion_variants`, `similarity`, `row_outputs`, `attn_maps`).
    `online_stride=s` (and `online_history=`, default 256; the `forward_videos` loop; HIP device): every call is
    `MMFMIL.forward_videos_online` -- each video evaluated over trailing windows (`online_windows`), so that a snippet's score depends
    on fewer than s snippets after it (this package's own semantics; the reference evaluates offline; the NaN rule stays per whole
    video).  The returned tuple holds the online scores and weight means; `score_loader.last_result` becomes {"online": {"scores": per
    video a [snippets] float32 array; "scores_device": ONE [N] device tensor of the N valid snippets, the videos in list order;
    "row_offsets": int64 array of len(videos) + 1 offsets into N; "stride", "history"}}.  The host-list walk does not take it: pass
    host_list=False (ValueError otherwise); it combines with none of the other extras."""
    on_gpu = torch.device(device).type == 'cuda'
    from .model import _row_output_keys, attn_map_layers, attn_maps_asked, fusion_variant_names, online_params
    variants = fusion_variant_names(fusion_variants)
    want_maps = attn_maps_asked(attn_maps)
    samples = None
    online = None
    if online_stride is not None:
        online = online_params(online_stride, online_history)
        if steps is not None or trajectory or variants or similarity or row_outputs is not None or want_maps or score_samples is not None:
            raise ValueError('online_stride does not combine with steps, trajectory, fusion_variants, score_samples, similarity, row_outputs or attn_maps')
        if host_list:
            raise ValueError('online_stride is not served by the host-list walk (iefvad_forward_videos_host has no online entry): '
                             'pass host_list=False for the forward_videos_online loop')
        if not (on_gpu and batch_chunks > 0 and hasattr(model, 'forward_videos_online')) or ragged is False:
            raise ValueError('online_stride takes the forward_videos_online loop: it needs a HIP device, batch_chunks > 0 and a model with '
                             'forward_videos_online (and not ragged=False)')
        ragged = True
    if score_samples is not None:
        if steps is not None or trajectory or variants or similarity or row_outputs is not None or want_maps:
            raise ValueError('score_samples does not combine with steps, trajectory, fusion_variants, similarity, row_outputs or attn_maps')
        if not hasattr(model, 'forward_samples'):
            raise ValueError('score_samples needs a model with forward_samples (iefvad_amd.MMFMIL)')
        if not on_gpu:
            raise ValueError('score_samples needs a HIP device')
        if sample_seed is None:
            raise ValueError('score_samples needs sample_seed=: the draws are a pure function of the seed')
        samples = (score_samples, sample_seed, sample_scale)
    if variants:
        if trajectory or similarity or row_outputs is not None or want_maps:
            raise ValueError('fusion_variants does not combine with trajectory, similarity, row_outputs or attn_maps')
        if not hasattr(model, 'set_steps'):
            raise ValueError('fusion_variants needs a model with the fusion_variants keyword (iefvad_amd.MMFMIL)')
        if not on_gpu:
            raise ValueError('fusion_variants needs a HIP device')
    if (steps is not None or trajectory) and not hasattr(model, 'set_steps'):
        raise ValueError('steps= and trajectory=True need a model with set_steps (iefvad_amd.MMFMIL)')
    if trajectory:
        if similarity or row_outputs is not None or want_maps:
            raise ValueError('trajectory=True does not combine with similarity, row_outputs or attn_maps')
        if not on_gpu:
            raise ValueError('trajectory=True needs a HIP device')
    row_keys = _row_output_keys(row_outputs)
    attn_layers = ()
    if want_maps:
        if similarity or row_outputs is not None:
            raise ValueError('attn_maps does not combine with similarity or row_outputs: iefvad_forward_videos_attn returns neither')
        if not (on_gpu and batch_chunks > 0 and hasattr(model, 'forward_videos')) or ragged is False:
            raise ValueError('attn_maps takes the forward_videos loop: it needs a HIP device, batch_chunks > 0 and a model with '
                             'forward_videos (and not ragged=False)')
        attn_layers = attn_map_layers(attn_maps, model.temporal.num_layers)
        ragged, host_list = True, False
    if row_outputs is not None:
        if similarity:
            raise ValueError('row_outputs does not combine with similarity: reduce the returned rows with similarity_rows')
        if not (on_gpu and batch_chunks > 0 and hasattr(model, 'forward_videos')) or ragged is False:
            raise ValueError('row_outputs takes the valid-row routes: it needs a HIP device, batch_chunks > 0 and a model with '
                             'forward_videos (and not ragged=False)')
        ragged = True
    sim_rows = isinstance(similarity, str)
    if sim_rows:
        if similarity != "rows":
            raise ValueError(f'similarity must be False, True (the padded route) or "rows" (the valid-row routes), got {similarity!r}')
        if not (on_gpu and batch_chunks > 0 and hasattr(model, 'forward_videos')) or ragged is False:
            raise ValueError('similarity="rows" takes the valid-row routes: it needs a HIP device, batch_chunks > 0 and a model with '
                             'forward_videos (and not ragged=False)')
        ragged = True
    elif similarity:
        if ragged:
            raise ValueError("similarity=True takes the padded route: ragged=True returns no fused / image_mu / event_mu")
        if getattr(model, 'outputs', 'full') != 'full':
            raise ValueError(_NEEDS_FULL)
        ragged = False
    nl = lanes if (on_gpu and lanes > 1 and hasattr(model, 'lanes')) else 1
    models = model.lanes(nl) if nl > 1 else [model]
    if ragged is None:
        ragged = on_gpu and batch_chunks > 0 and skip_empty_chunks and hasattr(model, 'forward_videos')
    elif ragged and not (on_gpu and batch_chunks > 0 and hasattr(model, 'forward_videos')):
        raise ValueError("ragged=True needs a HIP device, batch_chunks > 0 and a model with forward_videos")
    use_list = bool(ragged and host_list and hasattr(model, 'forward_videos_host'))
    if trajectory and use_list:
        raise ValueError('trajectory=True is not served by the host-list walk (iefvad_forward_videos_host has no trajectory entry): '
                         'pass host_list=False for the forward_videos loop')
    if variants and use_list:
        raise ValueError('fusion_variants is not served by the host-list walk (iefvad_forward_videos_host has no variants entry): '
                         'pass host_list=False for the forward_videos loop')
    if samples is not None and use_list:
        raise ValueError('score_samples is not served by the host-list walk (iefvad_forward_videos_host has no samples entry): '
                         'pass host_list=False for the forward_videos loop')
    # staging buffers are pinned allocations: they live with the lane (model object) across calls, not with the call
    stagers = [None] * nl
    for k, m in enumerate(models if on_gpu else ()):
        cache = m.__dict__.setdefault("_stagers", {}) if hasattr(m, "__dict__") else {}
        key = ("rows" if ragged else "chunks", str(device))
        if key not in cache:
            cache[key] = _RowStager(device) if ragged else _PinnedStager(device)
        stagers[k] = cache[key]
    streams = [torch.cuda.Stream(device=device) for _ in range(nl)] if nl > 1 else [None]
    sink = _ScoreSink()
    if similarity:
        sink.dev_sim = []
    if row_outputs is not None:
        sink.dev_rows = {k: [] for k in row_keys}
    if attn_layers:
        sink.dev_rows = {"image_attn": [], "event_attn": []}
    if trajectory or variants or samples is not None:
        sink.dev_traj = []
    with torch.no_grad():
        for s in streams if nl > 1 else ():
            s.wait_stream(torch.cuda.current_stream(device))         # e.g. a `model.to(device)` still in flight
        prev_steps = getattr(model, '_steps', None)
        if steps is not None:
            model.set_steps(steps)
        try:
            if use_list:
                _score_rows_list(model, test_loader, sink, maxlen, dataset, label_map, batch_chunks, host_list_bytes, wire_bf16, sim_rows,
                                 row_keys)
            elif ragged:
                _score_rows_loop(models, stagers, streams, test_loader, sink, maxlen, dataset, label_map, batch_chunks, sim_rows, row_keys,
                                 attn_layers, trajectory, variants, samples, online)
            else:
                _score_padded(models, stagers, streams, test_loader, sink, maxlen, device, dataset, label_map, batch_chunks, skip_empty_chunks,
                              bool(similarity), trajectory, variants, samples)
            nsteps = getattr(model, 'steps', 0)
        finally:
            if steps is not None:
                model.set_steps(prev_steps)
        for s in streams if nl > 1 else ():
            torch.cuda.current_stream(device).wait_stream(s)
        if trajectory or variants or samples is not None or sink.dev_rows is not None or online is not None:
            offsets = np.concatenate([[0], np.cumsum([n for _, n in sink.spans])]).astype(np.int64)
        if sink.dev_traj:
            # the slots of every forward side by side, then the valid ones in video order (the padded route leaves gaps between the videos' slots)
            slots = [torch.cat([t[i] for t in sink.dev_traj], dim=1) for i in range(len(sink.dev_traj[0]))]
            if offsets[-1] != sink.total:
                idx = torch.from_numpy(np.concatenate([np.arange(o, o + n, dtype=np.int64) for o, n in sink.spans])).to(slots[0].device)
                slots = [t[:, idx] for t in slots]
        if trajectory:
            ls, dn = slots if sink.dev_traj else (torch.zeros(nsteps + 1, 0, device=device), torch.zeros(nsteps, 0, device=device))
            sc = torch.sigmoid(ls).contiguous()
            score_loader.last_result = {"trajectory": {
                "scores_steps": sc.cpu().numpy(), "delta_norm": dn.cpu().numpy(), "scores_steps_device": sc, "row_offsets": offsets}}
        elif variants:
            lv = slots[0] if sink.dev_traj else torch.zeros(len(variants), 0, device=device)
            sc = torch.sigmoid(lv).contiguous()
            host = sc.cpu().numpy()
            score_loader.last_result = {"variants": {
                "names": tuple(variants), "scores": [host[:, a:b] for a, b in zip(offsets[:-1], offsets[1:])], "scores_device": sc,
                "row_offsets": offsets}}
        elif samples is not None:
            ls, ms = slots if sink.dev_traj else (torch.zeros(samples[0], 0, device=device), torch.zeros(2, 0, device=device))
            host = ms.cpu().numpy()
            score_loader.last_result = {"samples": {
                "scores_mean": [host[0, a:b] for a, b in zip(offsets[:-1], offsets[1:])],
                "scores_std": [host[1, a:b] for a, b in zip(offsets[:-1], offsets[1:])],
                "logits_samples_device": ls.contiguous(), "row_offsets": offsets}}
        elif attn_layers:
            image, event = (v[0] if len(v) == 1 else torch.cat(v, dim=1) if v else torch.zeros(len(attn_layers), 0, maxlen, device=device)
                            for v in (sink.dev_rows["image_attn"], sink.dev_rows["event_attn"]))
            score_loader.last_result = {"attn_maps": {"image": image, "event": event, "layers": attn_layers, "row_offsets": offsets}}
        elif sink.dev_rows is not None:
            D = getattr(getattr(model, 'temporal', None), 'embed_dim', 0)
            score_loader.last_result = {
                # one library call (the host-list walk's usual case): its tensors as they are, no second copy
                "row_outputs": {k: v[0] if len(v) == 1 else torch.cat(v) if v else torch.zeros(0, D, device=device)
                                for k, v in sink.dev_rows.items()},
                "row_offsets": offsets}
        if online is not None:
            res = sink.finish(device, True)
            score_loader.last_result = {"online": {"scores": res[0], "scores_device": res[4], "row_offsets": offsets, "stride": online[0],
                                                   "history": online[1]}}
            return res if return_device else res[:4]
        return sink.finish(device, return_device)


class FeatureFilePipeline:
    """Streaming front end for real feature files.  The `.npy` headers are parsed first (shape
    and dtype without touching the payload), the chunks of consecutive videos are laid out into batches of
    >= `batch_chunks` chunks, and worker threads then read() each video's image / event payload STRAIGHT into its
    slot of a pinned host staging buffer (one copy, GIL released, in parallel); a finished batch goes to the
    device on a side stream, so file I/O, PCIe and the forward of the previous batch overlap.  Order is preserved.
    Semantics match the reference loader + test() prologue: dtype preserved from disk (dataset.py:37-38,49-50;
    a batch mixing dtypes is widened to fp32, which `.to(torch.float)` does anyway), conditional nan_to_num
    (test.py:90-95), and the all-zero trailing chunk of a len % 256 == 0 video is dropped (its rows are sliced
    away by test.py:121)."""

    def __init__(self, paths: Sequence[str], labels: Sequence[str], clip_dim: int, event_dir: str, device,
                 batch_chunks: int = 64, workers: int = 2, prefetch: int = 2, ragged: bool = False):
        self.paths, self.labels = list(paths), list(labels)
        self.clip_dim, self.event_dir, self.device = clip_dim, event_dir, torch.device(device)
        self.batch_chunks, self.workers, self.prefetch = batch_chunks, workers, max(1, prefetch)
        # ragged: batches are the videos' VALID rows only, [sum(len), D] per modality, for `MMFMIL.forward_videos`; no zero
        # padding is written and nothing on the host scans the payload (the NaN rule of test.py:90-95 runs on the device)
        self.ragged = ragged

    @staticmethod
    def _header(path):
        """(shape, dtype, payload offset) of a .npy file without touching the payload."""
        with open(path, 'rb') as f:
            ver = np.lib.format.read_magic(f)
            rd = np.lib.format.read_array_header_1_0 if ver == (1, 0) else np.lib.format.read_array_header_2_0
            shape, fortran, dtype = rd(f)
            if fortran or len(shape) != 2:
                raise ValueError(f"{path}: expected a C-ordered [len, D] array")
            return shape, dtype, f.tell()

    def _open(self, idx):
        p = self.paths[idx]
        pe = p.replace('rgb', self.event_dir)
        hi, he = self._header(p), self._header(pe)
        if tuple(hi[0]) != tuple(he[0]):
            # the reference would fail later, at the model's residual add of mismatched lengths; fail at the file
            raise ValueError(f"{pe}: event features {tuple(he[0])} do not match the image features {tuple(hi[0])} of {p}")
        return (p,) + hi, (pe,) + he

    @staticmethod
    def _fill(dst: np.ndarray, src, scan: bool = True):
        """One read() of the payload from the page cache straight into the pinned staging rows (no intermediate
        array, no page faults of a memory map); a dtype mismatch (mixed-dtype batch) goes through a temporary."""
        path, shape, dtype, offset = src
        with open(path, 'rb', buffering=0) as f:
            f.seek(offset)
            if dtype == dst.dtype:
                got = f.readinto(memoryview(dst.reshape(-1).view(np.uint8)))
                if got != dst.nbytes:
                    raise IOError(f"{path}: short read ({got} of {dst.nbytes} bytes)")
            else:
                tmp = np.fromfile(f, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
                np.copyto(dst, tmp, casting='unsafe')
        if not scan and dtype == dst.dtype:
            return            # ragged path, payload in its own dtype: the device decides (csrc/ragged.h)
        if np.issubdtype(dst.dtype, np.floating) and np.isnan(np.sum(dst, dtype=np.float32)) and np.isnan(dst).any():
            # conditional nan_to_num (test.py:90-95): NaN -> 0, +-inf -> the SOURCE dtype's max / min
            fi = np.finfo(dtype)
            np.nan_to_num(dst, copy=False, nan=0.0, posinf=float(fi.max), neginf=float(fi.min))

    @classmethod
    def _fill_many(cls, jobs, scan: bool = True):
        for dst, src in jobs:
            cls._fill(dst, src, scan)

    def batches(self):
        """Yields (img [B,T,D] device tensor, ev, [(video index, n snippets, n chunks), ...])."""
        from concurrent.futures import ThreadPoolExecutor
        T = self.clip_dim
        copy_stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None
        pin = self.device.type == 'cuda'
        with ThreadPoolExecutor(self.workers) as pool:
            maps = list(pool.map(self._open, range(len(self.paths))))      # headers only
            plans, cur, cur_chunks = [], [], 0
            for idx, (mi, _) in enumerate(maps):
                n = int(mi[1][0])
                nch = video_chunks(n, T)
                cur.append((idx, n, nch))
                cur_chunks += nch
                if cur_chunks >= self.batch_chunks:
                    plans.append(cur)
                    cur, cur_chunks = [], 0
            if cur:
                plans.append(cur)

            def start(plan):
                dts = {maps[i][0][2] for i, _, _ in plan} | {maps[i][1][2] for i, _, _ in plan}
                dt = np.dtype(np.float32) if len(dts) > 1 else next(iter(dts))
                D = int(maps[plan[0][0]][0][1][1])
                nchunks = sum(nch for _, _, nch in plan)
                tdt = torch.from_numpy(np.zeros(0, dt)).dtype
                if self.ragged:
                    nrows = sum(n for _, n, _ in plan)
                    hi = torch.empty(nrows, D, dtype=tdt, pin_memory=pin)
                    he = torch.empty(nrows, D, dtype=tdt, pin_memory=pin)
                    ni, ne = hi.numpy(), he.numpy()
                    jobs, off = [], 0
                    for idx, n, nch in plan:
                        jobs.append((ni[off:off + n], maps[idx][0]))
                        jobs.append((ne[off:off + n], maps[idx][1]))
                        off += n
                    nt = max(1, min(self.workers, len(jobs)))
                    return hi, he, [pool.submit(self._fill_many, jobs[w::nt], False) for w in range(nt)], plan
                hi = torch.empty(nchunks, T, D, dtype=tdt, pin_memory=pin)
                he = torch.empty(nchunks, T, D, dtype=tdt, pin_memory=pin)
                ni, ne = hi.numpy().reshape(-1, D), he.numpy().reshape(-1, D)
                futs, off = [], 0
                jobs = []
                for idx, n, nch in plan:
                    jobs.append((ni[off * T:off * T + n], maps[idx][0]))
                    jobs.append((ne[off * T:off * T + n], maps[idx][1]))
                    ni[off * T + n:(off + nch) * T] = 0          # zero padding of the video's last chunk only
                    ne[off * T + n:(off + nch) * T] = 0
                    off += nch
                # a few coarse tasks per batch: a page-cache read() runs at ~12 GB/s on one thread, so the Python
                # per-task overhead (and the GIL) of hundreds of tiny tasks would dominate
                nt = max(1, min(self.workers, len(jobs)))
                for w in range(nt):
                    futs.append(pool.submit(self._fill_many, jobs[w::nt]))
                return hi, he, futs, plan

            inflight = [start(p) for p in plans[:self.prefetch]]
            nxt = len(inflight)
            while inflight:
                hi, he, futs, plan = inflight.pop(0)
                for f in futs:
                    f.result()
                if nxt < len(plans):
                    inflight.append(start(plans[nxt]))
                    nxt += 1
                if copy_stream is not None:
                    with torch.cuda.stream(copy_stream):
                        di = hi.to(self.device, non_blocking=True)
                        de = he.to(self.device, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(copy_stream)
                    torch.cuda.current_stream(self.device).wait_event(done)
                    di.record_stream(torch.cuda.current_stream(self.device))
                    de.record_stream(torch.cuda.current_stream(self.device))
                else:
                    di, de = hi, he
                yield di, de, plan


def evaluate_files(args, model, gt, device, dataset: Optional[str] = None, batch_chunks: int = 64, workers: int = 2,
                   device_metrics: bool = True, verbose: bool = False):
    """End-to-end evaluation from a `path,label` CSV of feature files: streaming loader -> batched forward ->
    ordered scores -> AUC / AP (on the device when `device_metrics`).  Returns a dict with the metrics, the
    per-video scores and a wall-clock phase breakdown."""
    import time
    dataset = dataset or args.dataset
    with open(args.test_list, newline='') as f:
        rows = list(csv.DictReader(f))
    paths, labels = [r['path'] for r in rows], [r['label'] for r in rows]
    ragged = torch.device(device).type == 'cuda' and hasattr(model, 'forward_videos')
    pipe = FeatureFilePipeline(paths, labels, args.visual_length, EVENT_DIR[dataset], device, batch_chunks, workers,
                               ragged=ragged)
    model.eval()
    t0 = time.perf_counter()
    outs, metas = [], []
    with torch.no_grad():
        for img, ev, meta in pipe.batches():
            if ragged:       # valid rows only; chunker, NaN rule and [0:len] slicing on the device (csrc/ragged.h)
                outs.append(model.forward_videos(img, ev, [n for _, n, _ in meta])['logits'])
            else:
                o = model(img, ev, None, None, None)
                outs.append(o['logits'].reshape(img.shape[0], -1))
            metas.append(meta)
    T = args.visual_length
    pieces = []
    for lg, meta in zip(outs, metas):
        if ragged:
            pieces.append(lg)
            continue
        off = 0
        for _, n, nch in meta:
            pieces.append(lg[off:off + nch].reshape(-1)[:n])
            off += nch
    scores_dev = torch.sigmoid(torch.cat(pieces))
    if scores_dev.is_cuda:
        torch.cuda.synchronize(scores_dev.device)
    t1 = time.perf_counter()
    res: Dict[str, object] = {}
    device_metrics = device_metrics and scores_dev.is_cuda      # the metric kernels are the library's; a CPU run uses sklearn below
    if device_metrics:
        roc, ap = device_auc_ap(scores_dev, torch.as_tensor(gt))
        res.update(roc=roc, ap=ap)
    scores_host = scores_dev.float().cpu().numpy()
    t2 = time.perf_counter()
    lens = [n for meta in metas for _, n, _ in meta]
    offs = np.concatenate([[0], np.cumsum(lens)])
    per_video = [scores_host[offs[i]:offs[i + 1]] for i in range(len(lens))]
    if not device_metrics:
        res.update(evaluate_scores(per_video, labels, gt, dataset, verbose=verbose))
    res.update(scores=per_video, classes=labels, snippets=int(offs[-1]),
               seconds={"load+h2d+forward": t1 - t0, "metrics": t2 - t1})
    return res


# ------------------------------------------------------------------------------------------------
# vis=True: what the three test() files plot (test.py:177-207,276-328; ucf_test.py:181-211,219-333; xd_test.py:175-327)
# ------------------------------------------------------------------------------------------------
VIS_FRAMES = 3000      # frames per figure: a page of root test.py (chunk_size), the truncation of the train/ files
VIS_FLAVOURS = ("test", "ucf_test", "xd_test")


def vis_series(last_result: Dict[str, object], gt, flavour: str = "test", repeat: int = 16) -> Dict[str, Dict[str, object]]:
    """The data of every figure a vis=True run writes, keyed by file name -- a pure function of a `last_result` and the frame-level
    `gt`, so the plotted numbers can be checked without reading a PNG; `draw_vis` draws exactly this.

    Per class (first appearance in the list; the videos of a class concatenated in list order, every per-snippet series repeated
    x `repeat` to frames, gt = the class's frames of the running snippet offset, test.py:129):
      "test"                 pages of VIS_FRAMES frames, `{cls}_{page}.png` (page from 1): scores | w_i_mean, w_e_mean, the gt == 1 frames
                             as contiguous regions (first frame, last frame); root test.py draws no similarity figure (its call is
                             commented out, test.py:190)
      "ucf_test", "xd_test"  the first VIS_FRAMES frames only: `similarity_{cls}.png` cos_i, cos_e | dist_i, dist_e and `{cls}.png`
                             scores | w_i_mean, w_e_mean, the gt == 1 frames as marked points
    Each entry: {"x", "panels": [[(name, y), ...], [(name, y), ...]] (upper, lower), "gt_indices" (into x), "gt_regions" (list of
    (x_first, x_last), or None where points are marked), "title"}.  The title of a class figure carries the class ROC for an abnormal
    class that has one (`last_result["per_class"]`)."""
    if flavour not in VIS_FLAVOURS:
        raise ValueError(f"flavour must be one of {VIS_FLAVOURS}")
    gt = np.asarray(gt)
    classes = list(last_result["classes"])
    lens = [len(s) for s in last_result["scores"]]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    per_class = last_result.get("per_class", {})
    sim = last_result.get("similarity")

    def frames(per_video, members):
        return np.repeat(np.concatenate([np.asarray(per_video[v]).reshape(-1) for v in members]), repeat)

    out: Dict[str, Dict[str, object]] = {}
    for cls in dict.fromkeys(classes):
        members = [v for v, c in enumerate(classes) if c == cls]
        cls_gt = np.concatenate([gt[repeat * starts[v]:repeat * starts[v + 1]] for v in members])
        prob, wi, we = (frames(last_result[k], members) for k in ("scores", "w_i_mean", "w_e_mean"))
        roc = "" if cls in ('Normal', 'normal') or cls not in per_class else f" | ROC {per_class[cls][0]:.2f}"
        if flavour == "test":
            for page in range((len(prob) + VIS_FRAMES - 1) // VIS_FRAMES):
                a, b = page * VIS_FRAMES, min((page + 1) * VIS_FRAMES, len(prob))
                x = np.arange(a, b)
                idx = np.where(cls_gt[a:b] == 1)[0]
                runs = np.split(idx, np.where(np.diff(idx) != 1)[0] + 1) if idx.size else []
                out[f"{cls}_{page + 1}.png"] = {"x": x, "panels": [[("scores", prob[a:b])], [("w_i_mean", wi[a:b]), ("w_e_mean", we[a:b])]],
                                                "gt_indices": idx, "gt_regions": [(int(x[r[0]]), int(x[r[-1]])) for r in runs],
                                                "title": f"Class: {cls} Chunk {page + 1}{roc}"}
            continue
        n = min(len(prob), VIS_FRAMES)
        x = np.arange(n)
        idx = np.where(cls_gt[:n] == 1)[0]
        if sim is not None:
            ci, ce, di, de = (frames(sim[k], members)[:n] for k in SIMILARITY_KEYS)
            out[f"similarity_{cls}.png"] = {"x": x, "panels": [[("cos_i", ci), ("cos_e", ce)], [("dist_i", di), ("dist_e", de)]],
                                            "gt_indices": idx, "gt_regions": None, "title": f"Similarity Metrics over Time for Class {cls}"}
        out[f"{cls}.png"] = {"x": x, "panels": [[("scores", prob[:n])], [("w_i_mean", wi[:n]), ("w_e_mean", we[:n])]],
                             "gt_indices": idx, "gt_regions": None, "title": f"Class: {cls}{roc}"}
    return out


_VIS_LABELS = {"scores": "predicted probability", "w_i_mean": "$w_i$ (image)", "w_e_mean": "$w_e$ (event)",
               "cos_i": "cosine sim (fused, image)", "cos_e": "cosine sim (fused, event)",
               "dist_i": "Euclidean dist (fused, image)", "dist_e": "Euclidean dist (fused, event)"}
_VIS_COLOURS = {"scores": "gray", "w_i_mean": "skyblue", "cos_i": "skyblue", "dist_i": "skyblue"}


def draw_vis(series: Dict[str, Dict[str, object]], directory: str, dpi: float = 100) -> List[str]:
    """One two-panel 12 x 8 inch PNG per entry of `vis_series` under `directory` (created); returns the paths.  Figures are built on
    `matplotlib.figure.Figure` with an Agg canvas of their own: pyplot is not imported and the process's backend is not touched.
    A figure of 3,000 frames costs matplotlib 0.2 s (dpi 40) to 0.5 s (dpi 100) on the host, whatever the device did."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    os.makedirs(directory, exist_ok=True)
    paths = []
    for name, spec in series.items():
        fig = Figure(figsize=(12, 8), dpi=dpi)
        FigureCanvasAgg(fig)
        axs = fig.subplots(2, 1, sharex=True)
        fig.suptitle(spec["title"], fontsize=16)
        x, idx = spec["x"], spec["gt_indices"]
        for ax, panel in zip(axs, spec["panels"]):
            for key, y in panel:
                ax.plot(x, y, label=_VIS_LABELS[key], color=_VIS_COLOURS.get(key, "#90EE90"))
                if spec["gt_regions"] is None and len(idx):
                    ax.scatter(x[idx], y[idx], color="red", s=50)
            if spec["gt_regions"]:      # every region from its first to its last frame, as ONE collection (hundreds of patches per axis draw slowly)
                inside = np.zeros(len(x), bool)
                inside[idx] = True
                ax.fill_between(x, 0, 1, where=inside, transform=ax.get_xaxis_transform(), color="red", alpha=0.3, linewidth=0)
            ax.legend(loc="upper right")
            ax.grid(True)
        if spec["panels"][0][0][0] == "scores":
            axs[0].set_ylim(0, 1)
        axs[1].set_xlabel("frame")
        path = os.path.join(directory, name)
        fig.savefig(path, format="png")
        paths.append(path)
    return paths


def _run_test(args, model, test_loader, maxlen, gt, device, label_map, attn, vis, normal_keys, total_samples, log,
              batch_chunks, lanes, metric_tail="host", vis_flavour="test", vis_route="padded", attn_maps=None, steps=None, trajectory=False,
              fusion_variants=None, score_samples=None, sample_seed=None, online_stride=None, online_history=256):
    """The body the three `test()` functions of the reference share (test.py:57-212): model.to / eval, the per-video
    loop, the metric tail, the prints.  What differs between the files is passed in: the Ano-AUC filter, the
    "Total Samples" suffix of ucf_test.py:173-174 and the `wandb.log` calls (ucf_test.py:158-162,175-178 /
    xd_test.py:155-159,170-173), which go to `log` when the caller supplies one (wandb itself is out of scope).
    `metric_tail`: "host" = sklearn (`evaluate_scores`); "device" = the library's metric entries on the scores as the loop left them
    on the device (`evaluate_scores_device`).
    `vis`: the plots of the file named by `vis_flavour` (`vis_series` / `draw_vis`) under vis/{args.exp_name}/, at `args.vis_dpi` dots
    per inch where the namespace has one (100 otherwise); the result dict gains "similarity" (the four series of `similarity_rows`,
    per video) and "vis_files" (the PNG paths written).
    `vis_route` (read with vis=True only): "padded" = `score_loader(similarity=True)`, whole chunks through an outputs="full" model;
    "rows" = `score_loader(similarity="rows")`, the valid-row routes, any `outputs=`.  A vis evaluation is for plots, so with
    `batch_chunks` unset "rows" packs 64 chunks in EVERY arithmetic (bf16x6 / fp16x3: the scores move inside the fp32 gates, as below).
    `attn_maps` (True or encoder layer indices): passed on to `score_loader(attn_maps=...)` -- the `forward_videos` loop, 64 chunks per
    call with `batch_chunks` unset, as for "rows" -- and the result dict gains "attn_maps" (device tensors, see there).  It does not
    combine with vis=True (ValueError: the vis routes collect the similarity series).  `attn=True` is unrelated: it keeps returning the
    reference's empty list.
    `steps`: the evaluation runs only the first `steps` refinement blocks (`score_loader(steps=...)`).  `trajectory=True`: one walk
    gives the whole ablation -- `score_loader(trajectory=True)` on the per-video route or the `forward_videos` loop -- and the result
    dict gains "trajectory" (see there), "auc_steps" and "ap_steps": the global AUC / AP of the scores after k = 0 .. steps steps, by
    the metric tail in use (sklearn, or `iefvad_auc_ap`).  Entry k is what a `steps=k` evaluation returns; nothing more is printed.  It
    does not combine with vis=True or `attn_maps`.
    `fusion_variants` (True or names): one walk gives the fusion ablation table -- `score_loader(fusion_variants=...)` on the per-video
    route or the `forward_videos` loop -- and the result dict gains "variants" (see there), "auc_variants" and "ap_variants": name ->
    the global AUC / AP of that variant's scores, by the metric tail in use (sklearn, or `iefvad_auc_ap`).  "fused" is what the call
    itself returns; nothing more is printed.  It does not combine with vis=True, `attn_maps` or `trajectory`.
    `score_samples=S` with `sample_seed=`: one walk gives S Monte Carlo draws of every score from the heads' own Gaussians --
    `score_loader(score_samples=...)` on the per-video route or the `forward_videos` loop -- and the result dict gains "samples" (see
    there), "auc_samples" / "ap_samples" (S floats each: the global AUC / AP of sample s's scores) and "auc_mean_score" / "ap_mean_score"
    (those of the per-snippet mean score), by the metric tail in use; nothing more is printed.  It combines with none of the other extras.
    `online_stride=s` (with `online_history=`, default 256): IN ADDITION to the evaluation above, a second walk over the loader --
    `score_loader(online_stride=s, host_list=False)`, 64 chunks per call with `batch_chunks` unset or 0 -- scores every video over
    trailing windows (`MMFMIL.forward_videos_online`); the result dict gains "online" (see there), "auc_online" and "ap_online": the
    global AUC / AP of the online scores, by the metric tail in use (sklearn, or `iefvad_auc_ap`).  Nothing more is printed; the
    returned values and every other key are those of the same call without it.  The loader must be iterable twice."""
    from .model import attn_maps_asked, online_params
    if online_stride is not None:
        online_params(online_stride, online_history)
    want_maps = attn_maps_asked(attn_maps)
    if score_samples is not None and (vis or trajectory or want_maps or steps is not None or (fusion_variants is not None and fusion_variants is not False)):
        raise ValueError("score_samples does not combine with vis=True, attn_maps, steps, trajectory or fusion_variants")
    want_variants = fusion_variants is not None and fusion_variants is not False
    if want_variants and (vis or trajectory or want_maps):
        raise ValueError("fusion_variants does not combine with vis=True, attn_maps or trajectory")
    if trajectory and (vis or want_maps):
        raise ValueError("trajectory=True does not combine with vis=True or attn_maps")
    if metric_tail not in ("host", "device"):
        raise ValueError('metric_tail must be "host" or "device"')
    if vis_route not in ("padded", "rows"):
        raise ValueError(f'vis_route must be "padded" or "rows" (got {vis_route!r})')
    vis_rows = bool(vis) and vis_route == "rows"
    model.to(device)
    model.eval()
    if batch_chunks is None:
        # default of the three entries: the packed route (the list walked inside the library, valid rows only) wherever it gives the
        # SAME BITS as one forward per video -- compute "f32" (every tiling sums k in one order) and "bf16" (ring and row-block kernels
        # are bit-identical); "bf16x6" / "fp16x3" pick their kernels by batch size, so they keep the reference's per-video pattern unless
        # the caller asks (batch_chunks=64: scores move at the 1e-7 level, inside the fp32 gates).  Five times the per-video rate on a
        # UCF-sized list.
        # A "bf16x6" model built with batch_invariant=True runs one arithmetic at every batch size: packed gives its per-video bits too.
        compute = getattr(model, "compute", None)
        invariant = compute in ("f32", "bf16") or (compute == "bf16x6" and getattr(model, "batch_invariant", False))
        packed_same_bits = (invariant and torch.device(device).type == "cuda" and lanes == 1)
        batch_chunks = 64 if (packed_same_bits or vis_rows or want_maps) else 0
    # vis=True: the same loop with the four similarity series collected on the device (`score_loader(similarity=True)`, a last result)
    got = score_loader(model, test_loader, maxlen, device, args.dataset, label_map, batch_chunks, lanes=lanes,
                       return_device=metric_tail == "device", similarity="rows" if vis_rows else bool(vis),
                       **(dict(attn_maps=attn_maps) if want_maps else {}), **(dict(steps=steps) if steps is not None else {}),
                       **(dict(trajectory=True, host_list=False) if trajectory else {}),
                       **(dict(fusion_variants=fusion_variants, host_list=False) if want_variants else {}),
                       **(dict(score_samples=score_samples, sample_seed=sample_seed, host_list=False) if score_samples is not None else {}))
    scores, classes, wi, we = got[:4]
    if metric_tail == "device":
        res = evaluate_scores_device((got[4], [len(s) for s in scores]), classes, gt, args.dataset, verbose=True, normal_keys=normal_keys,
                                     total_samples=total_samples, log=log)
    else:
        res = evaluate_scores(scores, classes, gt, args.dataset, verbose=True, normal_keys=normal_keys,
                              total_samples=total_samples, log=log)
    last = dict(res, scores=scores, classes=classes, w_i_mean=wi, w_e_mean=we)
    if want_maps:
        last["attn_maps"] = score_loader.last_result["attn_maps"]
    if trajectory:
        tr = last["trajectory"] = score_loader.last_result["trajectory"]
        if metric_tail == "device":
            pairs = [device_auc_ap(row, gt) for row in tr["scores_steps_device"]]
        else:       # the calls of evaluate_scores (test.py:158-159) on each step's scores
            from sklearn.metrics import average_precision_score, roc_auc_score
            pairs = [(roc_auc_score(gt, np.repeat(row.tolist(), 16)), average_precision_score(gt, np.repeat(row.tolist(), 16)))
                     for row in tr["scores_steps"]]
        last["auc_steps"], last["ap_steps"] = [p[0] for p in pairs], [p[1] for p in pairs]
    if want_variants:
        va = last["variants"] = score_loader.last_result["variants"]
        if metric_tail == "device":
            pairs = [device_auc_ap(row, gt) for row in va["scores_device"]]
        else:       # the calls of evaluate_scores (test.py:158-159) on each variant's scores
            from sklearn.metrics import average_precision_score, roc_auc_score
            rows = np.concatenate(va["scores"], axis=1) if va["scores"] else np.zeros((len(va["names"]), 0), np.float32)
            pairs = [(roc_auc_score(gt, np.repeat(row.tolist(), 16)), average_precision_score(gt, np.repeat(row.tolist(), 16))) for row in rows]
        last["auc_variants"] = {n: p[0] for n, p in zip(va["names"], pairs)}
        last["ap_variants"] = {n: p[1] for n, p in zip(va["names"], pairs)}
    if score_samples is not None:
        sm = last["samples"] = score_loader.last_result["samples"]
        mean_host = np.concatenate(sm["scores_mean"]) if sm["scores_mean"] else np.zeros(0, np.float32)
        if metric_tail == "device":
            dev = sm["logits_samples_device"]
            pairs = [device_auc_ap(row, gt) for row in torch.sigmoid(dev)] + [device_auc_ap(torch.from_numpy(mean_host).to(dev.device), gt)]
        else:       # the calls of evaluate_scores (test.py:158-159) on each sample's scores, then on the mean score
            from sklearn.metrics import average_precision_score, roc_auc_score
            rows = list(torch.sigmoid(sm["logits_samples_device"]).cpu().numpy()) + [mean_host]
            pairs = [(roc_auc_score(gt, np.repeat(row.tolist(), 16)), average_precision_score(gt, np.repeat(row.tolist(), 16))) for row in rows]
        last["auc_samples"], last["ap_samples"] = [p[0] for p in pairs[:-1]], [p[1] for p in pairs[:-1]]
        last["auc_mean_score"], last["ap_mean_score"] = pairs[-1]
    if online_stride is not None:
        score_loader(model, test_loader, maxlen, device, args.dataset, label_map, batch_chunks if batch_chunks > 0 else 64, host_list=False,
                     online_stride=online_stride, online_history=online_history)
        on = last["online"] = score_loader.last_result["online"]
        if metric_tail == "device":
            last["auc_online"], last["ap_online"] = device_auc_ap(on["scores_device"], gt)
        else:       # the calls of evaluate_scores (test.py:158-159) on the online scores
            from sklearn.metrics import average_precision_score, roc_auc_score
            flat = np.repeat(np.concatenate(on["scores"]).tolist() if on["scores"] else [], 16)
            last["auc_online"], last["ap_online"] = roc_auc_score(gt, flat), average_precision_score(gt, flat)
    if vis:
        last["similarity"] = got[-1]
        last["vis_files"] = draw_vis(vis_series(last, gt, vis_flavour), os.path.join('vis', str(args.exp_name)),      # test.py:59-62
                                     dpi=getattr(args, 'vis_dpi', 100))
    if attn:     # the reference returns the empty list it never fills (test.py:73,209-210)
        return (res["roc"], res["ap"], [], classes), last
    return (res["roc"], res["ap"]), last


def test(args, model, test_loader, maxlen, prompt_text, gt, device, attn=False, vis=False, label_map=None,
         batch_chunks: Optional[int] = None, normal_keys=('Normal',), lanes: int = 1, metric_tail: str = "host", vis_route: str = "padded",
         *, attn_maps=None, steps=None, trajectory=False, fusion_variants=None, score_samples=None, sample_seed=None, online_stride=None,
         online_history=256):
    """Counterpart of ROOT `test.py`'s `test()` (test.py:46-56; call site test.py:380-390): same positional order
    (..., device, attn, vis), Ano-AUC over every class but 'Normal' (test.py:336).  `label_map` is keyword-only in
    spirit: root test.py reads a global for the xd remap (test.py:81).  Returns (ROC1, AP1), or
    (ROC1, AP1, attn_weights, labels) when attn=True.  For `train/ucf_test.py` and `train/xd_test.py` -- whose
    positional orders differ from this one and from each other -- use `ucf_test` / `xd_test` below.
    `metric_tail="device"` (opt-in, here and in `ucf_test` / `xd_test`): the whole metric tail -- global, Ano-AUC and per-class --
    through the library on the device-resident scores (`evaluate_scores_device`) instead of sklearn on the host.
    `vis_route="rows"` (opt-in, here and in `ucf_test` / `xd_test`): a vis=True evaluation on the valid-row routes (`_run_test`).
    `attn_maps=` (keyword-only, here and in `ucf_test` / `xd_test`): the encoder's head-averaged attention maps of every valid snippet
    in `last_result["attn_maps"]` (`_run_test`, `score_loader`); `attn=True` keeps returning the reference's empty list.
    `steps=` / `trajectory=True` (keyword-only, here and in `ucf_test` / `xd_test`): evaluate with the first `steps` refinement blocks
    only / add the per-step scores, update norms and "auc_steps", "ap_steps" to `last_result` from the one walk (`_run_test`).
    `fusion_variants=` (keyword-only, here and in `ucf_test` / `xd_test`): True or names; adds the fusion ablations' scores ("variants")
    and "auc_variants", "ap_variants" (name -> float) to `last_result` from the one walk (`_run_test`).
    `score_samples=S`, `sample_seed=` (keyword-only, here and in `ucf_test` / `xd_test`): adds the Monte Carlo score samples ("samples"),
    "auc_samples" / "ap_samples" (S floats each) and "auc_mean_score" / "ap_mean_score" to `last_result` from the one walk (`_run_test`).
    `online_stride=s`, `online_history=` (keyword-only, here and in `ucf_test` / `xd_test`): a second walk scores every video over
    trailing windows (`MMFMIL.forward_videos_online`) and adds "online", "auc_online" and "ap_online" to `last_result` (`_run_test`)."""
    ret, test.last_result = _run_test(args, model, test_loader, maxlen, gt, device, label_map, attn, vis, normal_keys,
                                      False, None, batch_chunks, lanes, metric_tail, vis_route=vis_route, attn_maps=attn_maps, steps=steps,
                                      trajectory=trajectory, fusion_variants=fusion_variants, score_samples=score_samples, sample_seed=sample_seed,
                                      online_stride=online_stride, online_history=online_history)
    return ret


def ucf_test(args, model, test_loader, maxlen, prompt_text, gt, device, attn=False, vis=False, *, log=None,
             batch_chunks: Optional[int] = None, lanes: int = 1, metric_tail: str = "host", vis_route: str = "padded", attn_maps=None,
             steps=None, trajectory=False, fusion_variants=None, score_samples=None, sample_seed=None, online_stride=None, online_history=256):
    """Drop-in for `train/ucf_test.py`'s `test` (ucf_test.py:16-26; call site ucf_train.py:130-139): positional order
    (..., device, attn, vis); Ano-AUC excludes BOTH 'Normal' and 'normal' (ucf_test.py:340); the per-class lines carry
    "Total Samples" (ucf_test.py:173-174).  `log` (e.g. `wandb.log`) receives the dicts the reference logs."""
    ret, ucf_test.last_result = _run_test(args, model, test_loader, maxlen, gt, device, None, attn, vis,
                                          ('Normal', 'normal'), True, log, batch_chunks, lanes, metric_tail, "ucf_test", vis_route, attn_maps, steps,
                                          trajectory, fusion_variants, score_samples, sample_seed, online_stride, online_history)
    test.last_result = ucf_test.last_result
    return ret


def xd_test(args, model, test_loader, maxlen, prompt_text, gt, device, label_map, vis=False, attn=False, *, log=None,
            batch_chunks: Optional[int] = None, lanes: int = 1, metric_tail: str = "host", vis_route: str = "padded", attn_maps=None,
            steps=None, trajectory=False, fusion_variants=None, score_samples=None, sample_seed=None, online_stride=None, online_history=256):
    """Drop-in for `train/xd_test.py`'s `test` (xd_test.py:15-26; call site xd_train.py:102-112): `label_map` is the
    8th positional, then (vis, attn) -- the reverse of ucf_test's order; every video's class is
    `label_map[cls.split('-')[0]]` whatever args.dataset says (xd_test.py:68, unconditional); Ano-AUC excludes
    'normal' only (xd_test.py:334)."""
    if label_map is None:
        raise TypeError("xd_test: label_map is required (xd_test.py:68 indexes it for every video)")
    ret, xd_test.last_result = _run_test(args, model, test_loader, maxlen, gt, device, _AlwaysRemap(label_map), attn, vis,
                                         ('normal',), False, log, batch_chunks, lanes, metric_tail, "xd_test", vis_route, attn_maps, steps, trajectory,
                                         fusion_variants, score_samples, sample_seed, online_stride, online_history)
    test.last_result = xd_test.last_result
    return ret


class _AlwaysRemap(dict):
    """Marks a label map whose remap applies for every dataset name (xd_test.py:68) -- `harness.test` applies it for
    args.dataset == 'xd' only, as root test.py:80-81 does."""


# ------------------------------------------------------------------------------------------------
# robustness sweep -- the second inference caller of the forward (/root/reference/test2.py:35-123, levels :29-32)
# ------------------------------------------------------------------------------------------------
SWEEP_LEVELS = (0, 0.05, 0.1, 0.2, 0.3, 0.5)      # fraction of a chunk's time steps that gets attenuated


def sweep_plan():
    """(name, sigma_img, sigma_ev) for the twelve runs of the reference's sweep: every level on the image features
    with the event features untouched, then the other way round."""
    return ([("IMG_NOISE", s, 0) for s in SWEEP_LEVELS] + [("EV_NOISE", 0, s) for s in SWEEP_LEVELS])


def noise_plan():
    """(name, keyword arguments of `PerturbationSweep.level`) for the noise study the reference's flags promise and never run
    (test2.py:214-220; semantics defined by this package, "parity unpinned"): the six SWEEP_LEVELS as Gaussian sigma per modality, as
    outlier ratio per modality, and as modality-drop probability."""
    plan = []
    for key, name in (("noise_sigma_img", "IMG_GAUSS"), ("noise_sigma_ev", "EV_GAUSS"), ("outlier_img", "IMG_OUTLIER"),
                      ("outlier_ev", "EV_OUTLIER"), ("dropout_prob", "MODALITY_DROP")):
        plan += [(name, {key: s}) for s in SWEEP_LEVELS]
    return plan


_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(x):
    """murmur3's 32-bit finaliser on uint64 arrays holding 32-bit values (csrc/common.h, fmix32)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x ^ (x >> np.uint64(16))


def dropout_bits(seed: int, idx):
    """Host model of the library's counter-based 24-bit generator (csrc/common.h, dropout_bits): `idx` a uint64 array."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & _M32, idx >> np.uint64(32)
    a = _fmix32(lo ^ np.uint64(seed & 0xFFFFFFFF))
    return _fmix32((a + np.uint64(seed >> 32) + hi * np.uint64(0x9E3779B1)) & _M32) >> np.uint64(8)


def gaussian_rows(seed: int, modality: int, row_ids, D: int) -> np.ndarray:
    """Host model of the library's row noise (include/iefvad.h, `iefvad_perturb`; csrc/common.h, gauss_pair): eps[len(row_ids), D] fp32,
    a standard normal that is a pure function of (seed, modality, noise id, column).  Columns come in pairs (2q, 2q + 1) by Box-Muller
    from two draws of `dropout_bits` at idx = ((id * 2 + modality) << 11) | (q << 1) and idx | 1; fp64 throughout, rounded once to fp32
    (the device computes in fp32: tests/test_gpu_perturb.py measures the difference)."""
    ids = np.asarray(row_ids, dtype=np.uint64).reshape(-1, 1)
    q = np.arange(D // 2, dtype=np.uint64).reshape(1, -1)
    idx = ((ids * np.uint64(2) + np.uint64(modality)) << np.uint64(11)) | (q << np.uint64(1))
    b1 = dropout_bits(seed, idx).astype(np.float64)
    b2 = dropout_bits(seed, idx | np.uint64(1)).astype(np.float64)
    u1, u2 = (b1 + 1.0) * 2.0 ** -24, b2 * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    eps = np.empty((ids.shape[0], D), dtype=np.float64)
    eps[:, 0::2] = rho * np.cos(2.0 * np.pi * u2)
    eps[:, 1::2] = rho * np.sin(2.0 * np.pi * u2)
    return eps.astype(np.float32)


def sweep_row_perturbation(lengths: Sequence[int], plans, T: int, noise_sigma=(0.0, 0.0), outlier_sigma: float = 1.0,
                           nchunks: Optional[Sequence[int]] = None, first_ids: Optional[Sequence[int]] = None):
    """The row vectors of one level of the noise study over the listed videos -> ((scale_img, scale_ev), (amp_img, amp_ev), ids), fp32
    host tensors (ids: int32), None where a modality has nothing of the kind.  `plans[v]` = (att, out, drop): `att` / `out` the pairs
    (image, event) of time steps drawn for attenuation (scale 0.01, test2.py:70-77) and for outliers (amplitude `outlier_sigma` instead of
    `noise_sigma[m]`), None where not drawn; `drop` the dropped modality (0 image, 1 event: scale 0 on all its valid rows) or None.
    `nchunks` None: the packed valid rows (sum(lengths) elements, ids None: the valid-row call numbers its rows itself).  `nchunks[v]`
    given: the padded layout, nchunks[v] * T rows per video -- pad rows get amplitude 0 and, for a dropped modality, keep scale 1 -- and
    ids = first_ids[v] + the snippet's index in its video (0 on pad rows, which carry no noise)."""
    padded = nchunks is not None
    want_scale = [any(p[0][m] is not None and p[0][m].numel() for p in plans) or any(p[2] == m for p in plans) for m in (0, 1)]
    want_amp = [noise_sigma[m] != 0 or any(p[1][m] is not None and p[1][m].numel() for p in plans) for m in (0, 1)]
    scale, amp, ids = ([], []), ([], []), []
    for v, (n, (att, out, drop)) in enumerate(zip(lengths, plans)):
        n = int(n)
        rows = int(nchunks[v]) * T if padded else n
        reps = -(-rows // T)
        for m in (0, 1):
            if want_scale[m]:
                step = torch.ones(T)
                if att[m] is not None and att[m].numel():
                    step[att[m]] = 0.01
                sc = step.repeat(reps)[:rows].clone()
                if drop == m:
                    sc[:n] = 0.0
                scale[m].append(sc)
            if want_amp[m]:
                step = torch.full((T,), float(noise_sigma[m]))
                if out[m] is not None and out[m].numel():
                    step[out[m]] = float(outlier_sigma)
                a = step.repeat(reps)[:rows].clone()
                a[n:] = 0.0
                amp[m].append(a)
        if padded:
            i = torch.zeros(rows, dtype=torch.int32)
            i[:n] = torch.arange(int(first_ids[v]), int(first_ids[v]) + n, dtype=torch.int32)
            ids.append(i)
    cat = lambda parts: torch.cat(parts).contiguous() if parts else None
    return ((cat(scale[0]), cat(scale[1])), (cat(amp[0]), cat(amp[1])), cat(ids) if padded and any(want_amp) else None)


def perturb_rows_host(x: torch.Tensor, scale, amp, seed, modality: int, ids) -> torch.Tensor:
    """The CPU plumbing path's perturbed copy of [rows, D] features, with torch ops: `x * scale` where the scale is not 1, then
    `x + amp * eps` (fp32 sum, rounded to x's dtype) where the amplitude is not 0, eps = `gaussian_rows(seed, modality, ids, D)`."""
    if scale is not None:
        x = torch.where((scale != 1)[:, None], x * scale[:, None].to(x.dtype), x)
    if amp is not None:
        eps = torch.from_numpy(gaussian_rows(seed, modality, ids.numpy(), x.shape[-1]))
        x = torch.where((amp != 0)[:, None], (x.float() + amp[:, None] * eps).to(x.dtype), x)
    return x


SAMPLE_SEED_STEP = 0x9E3779B97F4A7C15      # csrc/iefvad.hip, sample_seed


def sample_seed(seed: int, s: int) -> int:
    """The generator's seed of score sample `s` of a call seeded `seed` (include/iefvad.h, `iefvad_samples`): seed + s * 0x9E3779B97F4A7C15
    mod 2^64, the one definition the library and this host model share."""
    return (int(seed) + int(s) * SAMPLE_SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def sample_states_host(mu_i, lv_i, mu_e, lv_e, seed: int, s: int, ids, factor: float, eps: float, scale: float = 1.0) -> torch.Tensor:
    """Host model (torch, fp64) of the sampled fused state z0_s of `MMFMIL.forward_samples` (csrc/samples.h): [rows, D] head tensors and
    the rows' snippet ids -> [rows, D] float64.  Noise = `gaussian_rows(sample_seed(seed, s), m, ids, D)`, sd_m = scale exp(0.5 lv_m) /
    sqrt(factor), mu~_m = mu_m + noise sd_m, and the fusion of the sampled means under the call's own precisions w_m = factor exp(-lv_m)
    with the reference's expression (imf_vad.py:130-144); `factor` the Student-t factor (nu + 1) / nu or 1, `eps` the fusion's epsilon."""
    mu_i, lv_i, mu_e, lv_e = (torch.as_tensor(np.asarray(t)).double() for t in (mu_i, lv_i, mu_e, lv_e))
    D = mu_i.shape[-1]
    ids = np.asarray(ids).reshape(-1)
    shape = mu_i.shape
    noise = [torch.from_numpy(gaussian_rows(sample_seed(seed, s), m, ids, D)).double().reshape(shape) for m in (0, 1)]
    root = math.sqrt(factor)
    mt_i = mu_i + noise[0] * (scale * torch.exp(0.5 * lv_i) / root)
    mt_e = mu_e + noise[1] * (scale * torch.exp(0.5 * lv_e) / root)
    w_i = factor * torch.exp(-lv_i)
    w_e = factor * torch.exp(-lv_e)
    den = w_i + w_e + eps
    return (w_i / den) * mt_i + (w_e / den) * mt_e


class SweepResult(tuple):
    """The 12 numbers `run_test` returns (test2.py:119-123), in its order, with names."""
    FIELDS = ("brier", "kl", "w_img_mean", "w_ev_mean", "auc", "ap", "w_img_anomalous", "w_ev_anomalous",
              "w_img_normal", "w_ev_normal", "w_img_change", "w_ev_change")

    def __getattr__(self, name):
        try:
            return self[self.FIELDS.index(name)]
        except ValueError:
            raise AttributeError(name) from None


def sweep_row_scales(lengths: Sequence[int], draws, T: int):
    """The two packed row-scale vectors (image, event; fp32 host tensors of sum(lengths) elements) of one level of the sweep on the
    valid-row route: row r of video v gets 0.01 if `r % T` is among the time steps `draws[v][m]` drawn for that video and modality,
    1 otherwise -- the `x[:, idx]` of test2.py:73,77 (every chunk of the video, the drawn time steps) restricted to the valid rows.
    A modality with no draw in any video gives None."""
    out = []
    for m in (0, 1):
        if all(d[m] is None or d[m].numel() == 0 for d in draws):
            out.append(None)
            continue
        parts = []
        for n, d in zip(lengths, draws):
            step = torch.ones(T)
            if d[m] is not None and d[m].numel():
                step[d[m]] = 0.01
            parts.append(step.repeat(-(-int(n) // T))[:int(n)])
        out.append(torch.cat(parts).contiguous())
    return out


class PerturbationSweep:
    """Robustness sweep over one test list, organised for the device instead of per video:

      * the videos are unpacked once (shape rule and unconditional `nan_to_num` of test2.py:52-60), packed across videos into
        batches of >= `batch_chunks` chunks (chunks are independent batch rows) and UPLOADED ONCE: the packed clean features stay
        resident on the device for all twelve levels;
      * the CLEAN pass -- identical for all twelve levels -- runs once; what later levels need from it stays on the
        device: the clean probabilities, and the per-dimension sums of the clean fusion weights;
      * a level draws its attenuated time steps with `torch.randperm(T)` once per video and modality, image first, in
        list order -- the draw sequence of test2.py:71-77, so seeding torch reproduces the reference's subsets -- and turns
        them into one fp32 row-scale vector per batch and modality (0.01 at the drawn time steps of every chunk of the video, as
        `x[:, idx]` does, 1 elsewhere) that the library applies in its input load (`iefvad_forward_scaled`): the clean
        features are never copied or modified;
      * the per-snippet means of the fusion weights come from the kernels (`w_i_mean`, `w_e_mean`); the full `w_i` / `w_e`
        are read only for the per-dimension sums of `w_img_change` / `w_ev_change` (test2.py:86-87);
      * Brier score, KL divergence, ROC-AUC / AP (`iefvad_auc_ap`) and the weight statistics are reduced on the device
        from per-snippet values and the 16-frames-per-snippet ground truth, never materialising the x16 repeat.

    On a HIP device `model` should be built with outputs="weights" (or "full").  With a CPU `device` (plumbing runs with a CPU
    model) the scale is applied to a copy with torch ops and the metrics come from sklearn as in test2.py:105-106.

    `ragged=True` (HIP only; the default is the padded route above) is the valid-row route of the evaluation loops
    (`MMFMIL.forward_videos`, csrc/ragged.h): only the VALID rows of every item are kept, concatenated in list order and uploaded
    once (`self.rows`); no padding crosses the boundary or is computed behind the encoder.  The unconditional `nan_to_num` is the
    library's mode "always", a level's draws become two packed scale vectors (`sweep_row_scales`), ONE `forward_videos` call per
    level serves the whole list, and the per-dimension weight sums come from the library's column-sum kernels (`w_colsum`), so a
    model built with outputs="scores" is enough.  The draws and the statistics are those of the padded route."""

    def __init__(self, args, model, loader, gt, device, batch_chunks: int = 64, repeat: int = 16, ragged: bool = False):
        self.model, self.device, self.repeat = model, torch.device(device), repeat
        self.T = T = args.visual_length
        self.ragged = bool(ragged)
        if self.ragged:
            if self.device.type != 'cuda':
                raise ValueError("PerturbationSweep(ragged=True) is the valid-row route of the HIP library (iefvad_forward_videos_scaled): "
                                 f"it runs on a HIP device only, not on {self.device}")
            self._init_rows(loader, gt)
            return
        videos: List[Tuple[torch.Tensor, torch.Tensor, int]] = []
        for item in loader:
            img, ev, n = item[0].squeeze(0), item[1].squeeze(0), int(item[3])
            if n < T:
                img, ev = img.unsqueeze(0), ev.unsqueeze(0)
            videos.append((torch.nan_to_num(img), torch.nan_to_num(ev), n))
        self.lengths = [n for _, _, n in videos]
        self.nchunks = [int(v[0].shape[0]) for v in videos]
        self.batches: List[List[int]] = [[]]
        load = 0
        for v, nch in enumerate(self.nchunks):
            self.batches[-1].append(v)
            load += nch
            if load >= batch_chunks and v + 1 < len(videos):
                self.batches.append([])
                load = 0
        # packed batches, resident on the device: (img [C, T, D], ev [C, T, D], valid row indices)
        self.packed = []
        for batch in self.batches:
            dts = {videos[v][m].dtype for v in batch for m in (0, 1)}
            dt = torch.float32 if len(dts) > 1 else next(iter(dts))
            img = torch.cat([videos[v][0].to(dt) for v in batch]).to(self.device)
            ev = torch.cat([videos[v][1].to(dt) for v in batch]).to(self.device)
            valid, off = [], 0
            for v in batch:
                valid.append(torch.arange(off * T, off * T + self.lengths[v]))
                off += self.nchunks[v]
            self.packed.append((img, ev, torch.cat(valid).to(self.device)))
        self._init_gt(gt)

    def _init_gt(self, gt):
        self.total = sum(self.lengths)
        g = torch.as_tensor(np.asarray(gt)[: self.repeat * self.total], dtype=torch.float64).reshape(self.total, self.repeat)
        self.gt = g.to(self.device)
        self.pos = self.gt.sum(dim=1)                        # anomalous frames of each snippet
        self.clean_passes = 0
        self._clean = None

    def _init_rows(self, loader, gt):
        """Valid-row route: the first `n` rows of every item, concatenated in list order, one upload per modality."""
        imgs, evs, self.lengths = [], [], []
        for item in loader:
            n = int(item[3])
            D = item[0].shape[-1]
            imgs.append(item[0].reshape(-1, D)[:n])
            evs.append(item[1].reshape(-1, D)[:n])
            self.lengths.append(n)
        dts = {t.dtype for t in imgs + evs}
        dt = torch.float32 if len(dts) > 1 else next(iter(dts))       # fp16 stays fp16, mixed dtypes widen to fp32
        self.rows = tuple(torch.cat([t.to(dt) for t in parts]).contiguous().to(self.device) for parts in (imgs, evs))
        self._init_gt(gt)

    def _pass_rows(self, draws=None, noise=None, rows=None):
        """One `forward_videos` call over the whole list: mode "always" of the NaN rule, the level's packed scale vectors, the
        column sums of the fusion weights from the device.  `noise` = (plans, sigmas, outlier_sigma, seed): a level of the noise study,
        its packed scale and amplitude vectors (`sweep_row_perturbation`); the call numbers its packed rows itself, which is the
        snippet's index in the list.  `rows`: other device rows than the resident clean ones (tools/perturb_probe.py: a copy perturbed
        on the host)."""
        rows = self.rows if rows is None else rows
        scale, kw = None, {}
        dev = lambda t: t.to(self.device) if t is not None else None
        if noise is not None:
            plans, sigmas, outlier_sigma, seed = noise
            sc, amp, _ = sweep_row_perturbation(self.lengths, plans, self.T, sigmas, outlier_sigma)
            scale = (dev(sc[0]), dev(sc[1]))
            if amp[0] is not None or amp[1] is not None:
                kw = dict(row_noise=(dev(amp[0]), dev(amp[1])), noise_seed=seed)
        elif draws is not None:
            si, se = sweep_row_scales(self.lengths, draws, self.T)
            scale = (si.to(self.device) if si is not None else None, se.to(self.device) if se is not None else None)
        with torch.no_grad():
            out = self.model.forward_videos(rows[0], rows[1], self.lengths, nan_to_num="always", row_scale=scale, weight_sums=True, **kw)
        return {"p": torch.sigmoid(out["logits"]).float(), "wi_row": out["w_i_mean"], "we_row": out["w_e_mean"],
                "wi_dim": out["w_colsum"][0] / self.total, "we_dim": out["w_colsum"][1] / self.total}

    def _scales(self, batch, draws):
        """Row-scale vectors [C * T] (image, event) of one packed batch for one level's draws; None for an untouched modality."""
        out = []
        C = sum(self.nchunks[v] for v in batch)
        for m in (0, 1):
            if all(draws[v][m] is None or draws[v][m].numel() == 0 for v in batch):
                out.append(None)
                continue
            sc = torch.ones(C, self.T)
            off = 0
            for v in batch:
                idx = draws[v][m]
                if idx is not None and idx.numel():
                    sc[off:off + self.nchunks[v], idx] = 0.01
                off += self.nchunks[v]
            out.append(sc.reshape(-1).to(self.device))
        return out

    # one packed pass over the list; `draws[v]` = (image time steps, event time steps) to attenuate in video v, or None
    def _pass(self, draws=None, noise=None):
        if self.ragged:
            return self._pass_rows(draws, noise)
        probs, wi_rows, we_rows = [], [], []
        wi_dim = we_dim = None
        on_gpu = self.device.type == 'cuda'
        first = np.concatenate([[0], np.cumsum(self.lengths)])       # a video's first snippet in the list: the noise ids
        with torch.no_grad():
            for batch, (img, ev, valid) in zip(self.batches, self.packed):
                if noise is not None:
                    plans, sigmas, outlier_sigma, seed = noise
                    sc, amp, ids = sweep_row_perturbation([self.lengths[v] for v in batch], [plans[v] for v in batch], self.T, sigmas,
                                                          outlier_sigma, [self.nchunks[v] for v in batch], [first[v] for v in batch])
                    if on_gpu:
                        dev = lambda t: t.to(self.device) if t is not None else None
                        kw = {}
                        if ids is not None:
                            kw = dict(row_noise=(dev(amp[0]), dev(amp[1])), noise_seed=seed, noise_rows=dev(ids))
                        out = self.model(img, ev, None, None, None, row_scale=(dev(sc[0]), dev(sc[1])), **kw)
                    else:       # CPU plumbing: the perturbed copy with torch ops and the host model of the generator
                        D = img.shape[-1]
                        xi = perturb_rows_host(img.reshape(-1, D), sc[0], amp[0], seed, 0, ids).reshape(img.shape)
                        xe = perturb_rows_host(ev.reshape(-1, D), sc[1], amp[1], seed, 1, ids).reshape(ev.shape)
                        out = self.model(xi, xe, None, None, None)
                elif draws is None:
                    out = self.model(img, ev, None, None, None)
                else:
                    si, se = self._scales(batch, draws)
                    if on_gpu:
                        out = self.model(img, ev, None, None, None, row_scale=(si, se))
                    else:       # CPU plumbing: the product as torch forms it on a copy (test2.py:70-77)
                        xi = img if si is None else (img * si.reshape(-1, self.T, 1).to(img.dtype))
                        xe = ev if se is None else (ev * se.reshape(-1, self.T, 1).to(ev.dtype))
                        out = self.model(xi, xe, None, None, None)
                D = out['w_i'].shape[-1]
                probs.append(torch.sigmoid(out['logits'].reshape(-1)[valid]).float())
                wi = out['w_i'].reshape(-1, D)[valid]
                we = out['w_e'].reshape(-1, D)[valid]
                wi_rows.append(out['w_i_mean'].reshape(-1)[valid] if 'w_i_mean' in out else wi.float().mean(dim=1))
                we_rows.append(out['w_e_mean'].reshape(-1)[valid] if 'w_e_mean' in out else we.float().mean(dim=1))
                si, se = wi.sum(dim=0, dtype=torch.float64), we.sum(dim=0, dtype=torch.float64)
                wi_dim = si if wi_dim is None else wi_dim + si
                we_dim = se if we_dim is None else we_dim + se
        return {"p": torch.cat(probs), "wi_row": torch.cat(wi_rows), "we_row": torch.cat(we_rows),
                "wi_dim": wi_dim / self.total, "we_dim": we_dim / self.total}

    def clean(self):
        if self._clean is None:
            self._clean = self._pass()
            self.clean_passes += 1
        return self._clean

    def _auc_ap(self, p):
        if self.device.type == 'cuda':
            return device_auc_ap(p, self.gt, self.repeat)
        from sklearn.metrics import average_precision_score, roc_auc_score      # test2.py:105-106
        y = np.repeat(p.cpu().numpy(), self.repeat)
        g = self.gt.reshape(-1).cpu().numpy()
        return roc_auc_score(g, y), average_precision_score(g, y)

    def level(self, sigma_img=0, sigma_ev=0, *, noise_sigma_img=0, noise_sigma_ev=0, outlier_img=0, outlier_ev=0, outlier_sigma=1.0,
              dropout_prob=0, noise_seed=None) -> SweepResult:
        """One level.  `sigma_img`, `sigma_ev`: the reference's attenuation (test2.py:70-77).  The keyword-only levels are the noise study
        whose flags the reference declares and never reads (test2.py:35-37,214-220); their semantics are defined here ("parity
        unpinned"), all on valid snippets only: `noise_sigma_*` -- every valid snippet of the modality gets x + sigma * eps, eps the
        library's standard normal (`gaussian_rows`); `outlier_*` = rho -- per video `torch.randperm(T)[:int(T * rho)]` time steps of
        every chunk get amplitude `outlier_sigma` instead; `dropout_prob` = p -- per video one `torch.rand(2)` draw u: if u[0] < p, the
        image modality (u[1] < 0.5) or the event modality gets row scale 0 on all its rows.  Draw order per video: the two attenuation
        draws, image outliers, event outliers, the drop draw, each only when its level is non-zero -- `level(sigma_img, sigma_ev)`
        consumes torch's RNG exactly as it always has.  With noise or outliers and `noise_seed=None`, one 63-bit seed is drawn from
        torch's RNG before the per-video draws.  Noise ids are the snippet's index in the list, on both routes."""
        c = self.clean()
        k_img, k_ev = int(self.T * sigma_img), int(self.T * sigma_ev)
        study = bool(noise_sigma_img or noise_sigma_ev or outlier_img or outlier_ev or dropout_prob)
        if (noise_sigma_img or noise_sigma_ev or outlier_img or outlier_ev) and noise_seed is None:
            noise_seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        draws, plans = [], []
        for _ in self.lengths:       # the reference's draw order: per video, image then event; no draw for a zero sigma
            di = torch.randperm(self.T)[:k_img] if sigma_img else None
            de = torch.randperm(self.T)[:k_ev] if sigma_ev else None
            draws.append((di, de))
            if study:
                oi = torch.randperm(self.T)[:int(self.T * outlier_img)] if outlier_img else None
                oe = torch.randperm(self.T)[:int(self.T * outlier_ev)] if outlier_ev else None
                drop = None
                if dropout_prob:
                    u = torch.rand(2)
                    if float(u[0]) < dropout_prob:
                        drop = 0 if float(u[1]) < 0.5 else 1
                plans.append(((di, de), (oi, oe), drop))
        n = self._pass(draws, (plans, (noise_sigma_img, noise_sigma_ev), outlier_sigma, noise_seed)) if study else self._pass(draws)
        return self._result(c, n)

    def _result(self, c, n) -> SweepResult:
        """run_test's 12 numbers (test2.py:89-123) from the clean pass `c` and a perturbed pass `n`"""
        rep = self.repeat
        yc, yn = c["p"].double(), n["p"].double()
        brier = ((yn[:, None] - self.gt) ** 2).mean()
        eps = 1e-8
        pc, qn = yc.clamp(eps, 1 - eps), yn.clamp(eps, 1 - eps)
        kl = (pc * torch.log(pc / qn) + (1 - pc) * torch.log((1 - pc) / (1 - qn))).mean()
        auc, ap = self._auc_ap(n["p"])
        wi, we = n["wi_row"].double(), n["we_row"].double()
        P, N = self.pos.sum(), (rep - self.pos).sum()
        stats = torch.stack([brier, kl, wi.mean(), we.mean(), (wi * self.pos).sum() / P, (we * self.pos).sum() / P,
                             (wi * (rep - self.pos)).sum() / N, (we * (rep - self.pos)).sum() / N]).cpu().tolist()
        return SweepResult((stats[0], stats[1], stats[2], stats[3], auc, ap, stats[4], stats[5], stats[6], stats[7],
                            (c["wi_dim"] - n["wi_dim"]).float().cpu(), (c["we_dim"] - n["we_dim"]).float().cpu()))


def run_perturbation_test(args, model, loader, gt, device, sigma_img=0, sigma_ev=0, clean_cache: Optional[dict] = None,
                          batch_chunks: int = 64, ragged: bool = False, *, noise_sigma_img=0, noise_sigma_ev=0, outlier_img=0, outlier_ev=0,
                          outlier_sigma=1.0, dropout_prob=0, noise_seed=None) -> SweepResult:
    """One level of the sweep with the call shape of the reference's `run_test(args, model, loader, gt, device,
    sigma_img, sigma_ev)` (test2.py:35) and its 12-tuple.  `clean_cache` (a dict the caller keeps across levels) holds
    the `PerturbationSweep`, so the unpacked list and the clean pass are shared by all levels.  `ragged=True`: the sweep's
    valid-row route (HIP only; `PerturbationSweep`).  The keyword-only levels are those of `PerturbationSweep.level`: the noise study of
    test2.py:214-220, which the reference declares and does not implement ("parity unpinned")."""
    model.eval()
    sweep = clean_cache.get("sweep") if clean_cache is not None else None
    if sweep is None:
        sweep = PerturbationSweep(args, model, loader, gt, device, batch_chunks, ragged=ragged)
        if clean_cache is not None:
            clean_cache["sweep"] = sweep
    return sweep.level(sigma_img, sigma_ev, noise_sigma_img=noise_sigma_img, noise_sigma_ev=noise_sigma_ev, outlier_img=outlier_img,
                       outlier_ev=outlier_ev, outlier_sigma=outlier_sigma, dropout_prob=dropout_prob, noise_seed=noise_seed)


# ------------------------------------------------------------------------------------------------
# multi-GPU: contiguous, snippet-balanced shards + one ordered score gather
# ------------------------------------------------------------------------------------------------
def partition_by_snippets(lengths: Sequence[int], world: int) -> List[Tuple[int, int]]:
    """Cut the ordered test list into `world` contiguous [begin, end) video ranges with ~equal snippet
    counts.  Contiguity keeps rank-order concatenation equal to the reference's sequential order, on
    which the gt offsets depend (test.py:129,153)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    total = int(lengths.sum())
    cum = np.concatenate([[0], np.cumsum(lengths)])
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        j = int(np.searchsorted(cum, target, side='left'))
        if j > 0 and abs(cum[j - 1] - target) <= abs(cum[min(j, len(cum) - 1)] - target):
            j -= 1
        j = min(max(j, cuts[-1]), len(lengths))
        cuts.append(j)
    cuts.append(len(lengths))
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


class ScoreComm:
    """The RCCL communicator of the score gather, owned by libiefvad (`iefvad_comm_*`, include/iefvad.h): created
    once per process over an initialised torch.distributed group, whose store only carries the 128-byte unique id
    from rank 0 to the other ranks.  The gather itself is `iefvad_gather_scores` on the caller's HIP stream."""

    CREATE_TIMEOUT_S = 120.0      # iefvad_comm_create is a collective (ncclCommInitRank): a rank that never arrives must not hang the job

    def __init__(self, device, group=None, create_timeout: Optional[float] = None, _hooks: Optional[dict] = None):
        """`_hooks` (tests only: tests/test_bench_launcher_cpu.py rehearses the failure paths on CPU ranks) replaces the four
        library calls of the handshake -- {'version', 'unique_id', 'create', 'destroy', 'nranks'} -- with callables."""
        import ctypes as C
        import threading
        import torch.distributed as dist
        from . import lib as _lib
        self._lib = _lib.load_library()
        self._last_error = _lib.last_error
        self._hooks = _hooks or {}
        self.device = torch.device(device)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        timeout = self.CREATE_TIMEOUT_S if create_timeout is None else float(create_timeout)
        # every failure below is made SYMMETRIC: a rank that raised alone would leave the others blocked in a collective.
        # First of all: can EVERY rank bind librccl?  (iefvad_comm_create is itself a collective -- ncclCommInitRank -- so a
        # rank that cannot even dlopen the library must be found out before anybody enters it.)
        version = self._hooks.get('version', lambda: int(self._lib.iefvad_rccl_version()))
        ver = torch.tensor([int(version())], dtype=torch.int64, device=self.device)
        dist.all_reduce(ver, op=dist.ReduceOp.MIN, group=group)
        if int(ver.item()) <= 0:
            raise RuntimeError("librccl cannot be bound on at least one rank (iefvad_rccl_version() == 0)")
        self.rccl_version = int(ver.item())
        ident = [None]
        if self.rank == 0:
            if 'unique_id' in self._hooks:
                ident = [self._hooks['unique_id']()]
            else:
                buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
                if self._lib.iefvad_comm_unique_id(buf) != 0:
                    ident = ["iefvad_comm_unique_id: " + self._last_error()]      # a str instead of the id: everybody raises
                else:
                    ident = [bytes(buf.raw)]
        dist.broadcast_object_list(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if not isinstance(ident[0], bytes):
            raise RuntimeError(str(ident[0]))
        self._h = C.c_void_p()
        # the collective create runs on a helper thread and is waited for with a deadline: if a peer died or never enters
        # ncclCommInitRank, this rank gives up after `timeout` seconds, reports failure in the all-reduce below -- which its
        # peers reach the same way -- and the job continues on torch.distributed's transport instead of hanging
        box = {}

        def create():
            try:
                if 'create' in self._hooks:
                    box['h'] = self._hooks['create'](ident[0], self.world, self.rank)
                    box['rc'] = 0
                else:
                    with torch.cuda.device(self.device):
                        box['rc'] = self._lib.iefvad_comm_create(C.c_char_p(ident[0]), self.world, self.rank, C.byref(self._h))
                    box['err'] = "" if box['rc'] == 0 else "iefvad_comm_create: " + self._last_error()     # thread-local message: read it here
            except Exception as e:       # noqa: BLE001 -- reported through the all-reduce like any other failure
                box['rc'], box['err'] = 1, f"iefvad_comm_create: {e}"

        th = threading.Thread(target=create, name="iefvad_comm_create", daemon=True)
        th.start()
        th.join(timeout)
        if th.is_alive():
            rc, err = 1, f"iefvad_comm_create did not return within {timeout:.0f} s (a peer never entered the collective)"
            self._abandoned = th       # still inside the collective: its handle is never used, the daemon thread dies with the process
        else:
            rc, err = box.get('rc', 1), box.get('err', "")
            if rc == 0 and 'h' in box:
                self._h = box['h']
        bad = torch.tensor([1 if rc != 0 else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=group)
        if int(bad.item()) != 0:
            if rc == 0:
                self.close()
            self._h = None
            raise RuntimeError(err or "iefvad_comm_create failed on another rank")
        self.nranks = int(self._hooks['nranks'](self._h)) if 'nranks' in self._hooks else int(self._lib.iefvad_comm_nranks(self._h))      # what RCCL reports

    def gather(self, local: torch.Tensor, counts: Optional[Sequence[int]] = None) -> torch.Tensor:
        import ctypes as C
        local = local.reshape(-1).float().contiguous()
        assert local.is_cuda and local.device == self.device
        if counts is None:
            counts = [local.numel()] * self.world
        assert len(counts) == self.world and counts[self.rank] == local.numel(), (counts, local.numel())
        out = torch.empty(int(sum(counts)), dtype=torch.float32, device=self.device)
        carr = (C.c_int64 * self.world)(*[int(c) for c in counts])
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = self._lib.iefvad_gather_scores(self._h, C.c_void_p(local.data_ptr()), local.numel(), carr,
                                                C.c_void_p(out.data_ptr()), out.numel(), st)
        if rc != 0:
            raise RuntimeError("iefvad_gather_scores: " + self._last_error())
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if 'destroy' in getattr(self, "_hooks", {}):
                self._hooks['destroy'](self._h)
            else:
                self._lib.iefvad_comm_destroy(self._h)
            self._h = None


_score_comms: Dict[object, ScoreComm] = {}


def gather_scores(local: torch.Tensor, group=None, counts: Optional[Sequence[int]] = None,
                  use_library: bool = True) -> torch.Tensor:
    """Rank-order concatenation of every rank's fp32 score vector, on every rank (= the reference's sequential
    order, test.py:123-129,153, because shards are contiguous ranges of the test list).

    `counts` are the per-rank lengths.  Every rank can compute them from the shared test list
    (`partition_by_snippets`), so pass them whenever possible: then nothing but the scores travels and nothing
    synchronises with the host -- equal counts are ONE all-gather.  Without `counts` the lengths are exchanged first
    (one small all-gather and a host read).
    HIP tensors on an "nccl" (= RCCL) group go through the library's own `iefvad_gather_scores`; CPU tensors (the
    gloo tests), and every tensor when `use_library` is False, through torch.distributed (`all_gather_into_tensor`,
    padded to the longest shard when the counts differ)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    local = local.reshape(-1).float()
    if counts is None:
        n = torch.tensor([local.numel()], dtype=torch.int64, device=local.device)
        allc = torch.empty(world, dtype=torch.int64, device=local.device)
        dist.all_gather_into_tensor(allc, n, group=group)
        counts = allc.tolist()
    counts = [int(c) for c in counts]
    if use_library and local.is_cuda and dist.get_backend(group) == "nccl":
        key = (group, local.device.index)
        if key not in _score_comms:
            _score_comms[key] = ScoreComm(local.device, group)
        return _score_comms[key].gather(local, counts)
    if len(set(counts)) == 1:
        out = torch.empty(world * counts[0], dtype=torch.float32, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
        return out
    mx = max(counts)
    buf = torch.zeros(mx, dtype=torch.float32, device=local.device)
    buf[:local.numel()] = local
    out = torch.empty(world * mx, dtype=torch.float32, device=local.device)
    dist.all_gather_into_tensor(out, buf, group=group)
    return torch.cat([out[r * mx:r * mx + counts[r]] for r in range(world)])


class ScoreGatherer:
    """How a multi-rank job gathers its score vectors, decided ONCE and by all ranks together: the library's RCCL gather
    (`ScoreComm` -> `iefvad_gather_scores`) when every rank can create the communicator -- `ScoreComm.__init__` fails on
    all ranks or on none -- else torch.distributed's `all_gather_into_tensor` (`gather_scores(use_library=False)`).
    `label` says which one runs.  There is no switch in mid-run: an enqueue error of the library gather on one rank would
    leave its peers inside the collective, so it propagates and ends the job instead of being papered over."""

    LIB = "iefvad_gather_scores (libiefvad -> librccl: ncclAllGather, or grouped ncclSend/ncclRecv for unequal shards, on the forward's stream)"
    TORCH = "torch.distributed all_gather_into_tensor"

    def __init__(self, device, group=None, prefer_library: bool = True, create_timeout: Optional[float] = None, _hooks=None):
        self.group, self.comm = group, None
        if prefer_library:
            try:
                self.comm = ScoreComm(device, group, create_timeout, _hooks)
                self.label = self.LIB
            except Exception as e:                  # symmetric (see ScoreComm.__init__): every rank lands here or none
                self.label = f"{self.TORCH} (library gather unavailable: {e})"
        else:
            self.label = self.TORCH

    def __call__(self, scores: torch.Tensor, counts: Optional[Sequence[int]] = None) -> torch.Tensor:
        if self.comm is not None:
            return self.comm.gather(scores, counts)
        return gather_scores(scores, self.group, counts, use_library=False)

    def close(self):
        if self.comm is not None:
            self.comm.close()
            self.comm = None


def shard_counts(lengths: Sequence[int], world: int) -> List[int]:
    """Snippets per rank under `partition_by_snippets` -- what every rank passes to `gather_scores(counts=...)`."""
    lengths = np.asarray(lengths, dtype=np.int64)
    return [int(lengths[a:b].sum()) for a, b in partition_by_snippets(lengths, world)]
