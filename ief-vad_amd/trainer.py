"""The reference's training loops over the MI355X path: counterparts of
/root/reference/train/ucf_train.py:16-156 (paired normal / abnormal batches: UCF-Crime, ShanghaiTech, MSAD) and
/root/reference/train/xd_train.py:14-129 (one loader: XD-Violence), with the same call signatures minus wandb.

One step = what ucf_train.py:43-106 does: `model.train()`, the conditional `nan_to_num` of the batch (:50-53), the forward
(`iefvad_train_forward`), CLAS2 + cosine / norm regulariser + Gaussian / Student-t KL (`iefvad_loss_forward`), `zero_grad`,
`loss.backward()` (`iefvad_loss_backward` then `iefvad_train_backward`), `optimizer.step()` (`iefvad_adamw_step`).  Around it the
loops keep the reference's bookkeeping: evaluation every `print_steps` samples through `harness.ucf_test` / `harness.xd_test`, the best checkpoint
(`{'epoch', 'model_state_dict', 'optimizer_state_dict', 'ap'}`, :141-149), `scheduler.step()` and the reload of the best
checkpoint at every epoch end (:151-153), the final rewrite as a bare state_dict (:155-156).  Logging goes to a callback instead
of wandb.  No torch op computes a loss or a gradient here.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, Optional, Sequence

import numpy as np
import torch
from torch.optim.lr_scheduler import MultiStepLR

from . import harness, losses


def get_prompt_text(label_map: dict) -> list:
    """train/utils.py:53-58: the label map's values, in order."""
    return list(label_map.values())


def get_batch_label(texts: Sequence[str], prompt_text: Sequence[str], label_map: dict) -> torch.Tensor:
    """One-hot (multi-hot for XD's 'a-b' labels) class vectors, the four cases of train/utils.py:5-50 keyed on the size of the label
    map exactly as the reference keys them: 17 entries (ShanghaiTech: 'normal' -> column 0, anything else column 1, two columns),
    2 entries (MSAD: 'Normal' -> 0), 7 entries (XD-Violence: every '-'-separated part that is in the map), otherwise (UCF-Crime:
    the column of the label's prompt text)."""
    n = len(label_map)
    if n == 17 or n == 2:
        normal = 'normal' if n == 17 else 'Normal'
        out = torch.zeros(len(texts), 2)
        for i, t in enumerate(texts):
            out[i, 0 if t == normal else 1] = 1
        return out
    out = torch.zeros(len(texts), len(prompt_text))
    for i, t in enumerate(texts):
        for part in (t.split('-') if n == 7 else [t]):
            if part in label_map:
                out[i, list(prompt_text).index(label_map[part])] = 1
    return out


def _nan_rule(x: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(x, nan=0.0) if bool(torch.isnan(x).any()) else x          # ucf_train.py:50-53


_NAN_FLAGS = {}


def _nan_rule_pair(img: torch.Tensor, ev: torch.Tensor):
    """ucf_train.py:50-53 for both inputs of a step.  fp32 device tensors go through `iefvad_nan_rule`: one scan + one repair launch,
    the flag never read by the host (torch's form costs an isnan pass, a reduction and a device-to-host wait per tensor and step);
    a tensor that does hold a NaN is repaired IN PLACE (the loops hand over per-step temporaries).  Anything else: the torch form."""
    ok = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 4 == 0 and t.data_ptr() % 16 == 0 for t in (img, ev))
    if not ok or img.numel() != ev.numel() or img.device != ev.device:
        return _nan_rule(img), _nan_rule(ev)
    import ctypes as C
    from . import lib as _lib
    dev = img.device
    flags = _NAN_FLAGS.get(dev)
    if flags is None:
        flags = _NAN_FLAGS[dev] = torch.zeros(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load_library().iefvad_nan_rule(C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()), img.numel(), C.c_void_p(flags.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError("iefvad_nan_rule: " + _lib.last_error())
    return img, ev


def train_step(model, optimizer, img: torch.Tensor, ev: torch.Tensor, labels: torch.Tensor, lengths: torch.Tensor,
               noise_model: str = "StudentT", lambda_reg: float = 1.0, lambda_kl: float = 1.0, nan_to_num: bool = True,
               want_terms: bool = True) -> Optional[Dict[str, torch.Tensor]]:
    """One optimiser step on a device batch; returns the eight loss terms (`losses.TERMS`) as 0-dim device tensors -- nothing
    is read back to the host -- or None with `want_terms=False` (the loops ask for them only on the steps they log:
    ucf_train.py:108-128 prints every `print_steps` samples)."""
    model.train()
    if nan_to_num:
        img, ev = _nan_rule_pair(img, ev)
    out = model(img, ev, None, None, lengths)
    nu = model.temporal.nu                                                             # ucf_train.py:94-95 reads it there
    total = losses.training_loss(out, labels, lengths, noise_model, nu, lambda_reg, lambda_kl)
    optimizer.zero_grad()
    total.backward()
    optimizer.step()
    if not want_terms:
        return None
    with torch.no_grad():
        terms = losses.training_losses({k: v.detach() for k, v in out.items()}, labels, lengths, noise_model, nu, lambda_reg, lambda_kl)
    return terms


def _save_best(path, epoch, model, optimizer, metric):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save({'epoch': epoch, 'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(), 'ap': metric}, path)


def _epoch_end(path, model, scheduler):
    scheduler.step()
    if os.path.exists(path):                     # the reference reloads the best weights after every epoch (ucf_train.py:151-153)
        ck = torch.load(path, weights_only=True)
        model.load_state_dict(ck['model_state_dict'])


def _finish(path):
    if os.path.exists(path):                     # ucf_train.py:155-156: the file ends up holding the bare state_dict
        ck = torch.load(path, weights_only=True)
        if 'model_state_dict' in ck:
            torch.save(ck['model_state_dict'], path)


def _check_vis_model(model, vis, vis_route="padded"):
    """The plots of a vis=True evaluation read `fused`, `image_mu` and `event_mu`: refuse a model that does not return them before
    the first step, not at the fifth epoch.  `vis_route="rows"` reduces the series inside the library (`harness.test`): any model."""
    if vis_route not in ("padded", "rows"):
        raise ValueError(f'vis_route must be "padded" or "rows" (got {vis_route!r})')
    if vis and vis_route == "padded" and getattr(model, "outputs", "full") != "full":
        raise ValueError(f'vis=True needs a model built with outputs="full" (this one has outputs="{model.outputs}")')


def train_paired(args, model, normal_loader, abnormal_loader, test_loader, label_map, device, gt: Optional[np.ndarray] = None,
                 log: Optional[Callable[[dict], None]] = None, optimizer=None, eval_batch_chunks: int = 64, vis: bool = False,
                 vis_route: str = "padded"):
    """Counterpart of /root/reference/train/ucf_train.py:train (same positional arguments; `gt` defaults to np.load(args.gt_path)).
    Each step concatenates a normal and an abnormal batch (:44-48), lambda_reg = lambda_kl = 1 (:100-101); the model is evaluated
    every `args.print_steps` samples and kept when its AUC improves.  Returns the best AUC.
    `vis=True`: an evaluation draws the reference's plots on its schedule (:138: every fifth epoch, past `args.vis_steps` samples);
    `vis_route="rows"` is passed on to `harness.ucf_test` (the valid-row routes; the model need not return the full dict)."""
    _check_vis_model(model, vis, vis_route)
    route_kw = {} if vis_route == "padded" else {"vis_route": vis_route}
    model.to(device)
    if gt is None:
        gt = np.load(args.gt_path)
    optimizer = optimizer or losses.AdamW(model.parameters(), lr=args.lr)
    scheduler = MultiStepLR(optimizer, args.scheduler_milestones, args.scheduler_rate)
    prompt_text = get_prompt_text(label_map)
    path = os.path.join('checkpoints', f'{args.exp_name}.pth')
    best = 0.0
    for e in range(args.max_epoch):
        n_it, a_it = iter(normal_loader), iter(abnormal_loader)
        for i in range(min(len(normal_loader), len(abnormal_loader))):
            n_img, n_ev, n_lab, n_len = next(n_it)
            a_img, a_ev, a_lab, a_len = next(a_it)
            img = torch.cat([n_img, a_img], dim=0).to(device)
            ev = torch.cat([n_ev, a_ev], dim=0).to(device)
            lengths = torch.cat([n_len, a_len], dim=0).to(device)
            labels = get_batch_label(list(n_lab) + list(a_lab), prompt_text, label_map).to(device)
            step = i * normal_loader.batch_size * 2                                    # ucf_train.py:42,106
            due = step % args.print_steps == 0 and step != 0
            terms = train_step(model, optimizer, img, ev, labels, lengths, args.noise_model, 1.0, 1.0, want_terms=due)
            if due:
                rec = {f'train/loss_{k}' if k != 'total' else 'train/loss': float(v) for k, v in terms.items()}
                auc, ap = harness.ucf_test(args, model, test_loader, args.visual_length, prompt_text, gt, device,   # ucf_train.py:130-139
                                           vis=bool(vis and (e + 1) % 5 == 0 and e > 0 and step > args.vis_steps),      # :138
                                           batch_chunks=eval_batch_chunks, **route_kw)
                rec.update(epoch=e, step=step, auc=auc, ap=ap)
                if log:
                    log(rec)
                if auc > best:
                    best = auc
                    _save_best(path, e, model, optimizer, best)
        _epoch_end(path, model, scheduler)
    _finish(path)
    return best


def train_single(args, model, train_loader, test_loader, label_map, device, gt: Optional[np.ndarray] = None,
                 log: Optional[Callable[[dict], None]] = None, optimizer=None, eval_batch_chunks: int = 64, vis: bool = False,
                 vis_route: str = "padded"):
    """Counterpart of /root/reference/train/xd_train.py:train: one loader, lambda_reg = lambda_kl = 0.01 (:73-74), the Student-t
    shift of the KL terms whatever `args.noise_model` says (:67-70 apply it unconditionally), best checkpoint by AP (:114).
    `vis=True`: an evaluation draws the reference's plots on its schedule (:111: every fifth epoch, past 33,000 samples);
    `vis_route="rows"` is passed on to `harness.xd_test`."""
    _check_vis_model(model, vis, vis_route)
    route_kw = {} if vis_route == "padded" else {"vis_route": vis_route}
    model.to(device)
    if gt is None:
        gt = np.load(args.gt_path)
    optimizer = optimizer or losses.AdamW(model.parameters(), lr=args.lr)
    scheduler = MultiStepLR(optimizer, args.scheduler_milestones, args.scheduler_rate)
    prompt_text = get_prompt_text(label_map)
    path = os.path.join('checkpoints', f'{args.exp_name}.pth')
    best = 0.0
    for e in range(args.max_epoch):
        for i, (img, ev, text_labels, lengths) in enumerate(train_loader):
            labels = get_batch_label(list(text_labels), prompt_text, label_map).to(device)
            step = i * train_loader.batch_size
            due = step % args.print_steps == 0 and step != 0
            terms = train_step(model, optimizer, img.to(device), ev.to(device), labels, lengths.to(device), "StudentT", 0.01, 0.01,
                               nan_to_num=False, want_terms=due)                        # xd_train.py has no NaN rule
            if due:
                rec = {f'train/loss_{k}' if k != 'total' else 'train/loss': float(v) for k, v in terms.items()}
                auc, ap = harness.xd_test(args, model, test_loader, args.visual_length, prompt_text, gt, device, label_map,   # xd_train.py:102-112
                                          vis=bool(vis and (e + 1) % 5 == 0 and e > 0 and step > 33000),      # :111
                                          batch_chunks=eval_batch_chunks, **route_kw)
                rec.update(epoch=e, step=step, auc=auc, ap=ap)
                if log:
                    log(rec)
                if ap > best:
                    best = ap
                    _save_best(path, e, model, optimizer, best)
        _epoch_end(path, model, scheduler)
    _finish(path)
    return best


# ------------------------------------------------------------------------------------------------
# the training set on the device (csrc/resample.h): windows formed once, a step's batch gathered by index
# ------------------------------------------------------------------------------------------------
_IN_CODES = {np.dtype(np.float32): 0, np.dtype(np.float16): 1}          # lib.IN_F32 / lib.IN_F16
_T = 256


def _stream(dev):
    import ctypes as C
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def resample_videos(rows: torch.Tensor, lengths: Sequence[int], out: Optional[torch.Tensor] = None,
                    out_lengths: Optional[torch.Tensor] = None):
    """`iefvad_resample_videos`: the packed rows [sum(lengths), D] (device, fp32 or fp16) of len(lengths) videos -> their windows
    [nv, 256, D] fp32 and int32 clip lengths, the reference's process_feat bit for bit (harness.process_feat is the host model)."""
    import ctypes as C
    from . import lib as _lib
    lens = [int(n) for n in lengths]
    nv, D = len(lens), int(rows.shape[-1])
    if not rows.is_cuda or not rows.is_contiguous() or rows.dim() != 2 or rows.shape[0] != sum(lens):
        raise ValueError(f"expected a contiguous [{sum(lens)}, D] device tensor (sum of lengths x D), got {tuple(rows.shape)}")
    code = {torch.float32: _lib.IN_F32, torch.float16: _lib.IN_F16}.get(rows.dtype)
    if code is None:
        raise ValueError(f"feature rows must be fp32 or fp16, got {rows.dtype}")
    dev = rows.device
    if out is None:
        out = torch.empty(nv, _T, D, dtype=torch.float32, device=dev)
    if out_lengths is None:
        out_lengths = torch.empty(nv, dtype=torch.int32, device=dev)
    for t, dt, shape in ((out, torch.float32, (nv, _T, D)), (out_lengths, torch.int32, (nv,))):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"resample_videos: out / out_lengths must be contiguous {dt} tensors of shape {shape} on {dev}")
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        ws = torch.empty(max(int(lib.iefvad_resample_workspace_bytes(nv)), 256), dtype=torch.uint8, device=dev)
        rc = lib.iefvad_resample_videos(C.c_void_p(rows.data_ptr()), code, (C.c_int32 * nv)(*lens), nv, _T, D, C.c_void_p(ws.data_ptr()),
                                        ws.numel(), C.c_void_p(out.data_ptr()), C.c_void_p(out_lengths.data_ptr()), _stream(dev))
    if rc != 0:
        raise RuntimeError("iefvad_resample_videos: " + _lib.last_error())
    return out, out_lengths


def gather_windows(img_set: torch.Tensor, ev_set: torch.Tensor, set_lengths: torch.Tensor, index):
    """`iefvad_gather_windows`: fresh tensors (img [B, 256, D], ev [B, 256, D], lengths int32 [B]) holding windows `index` of the two
    sets.  `index` is checked HERE, on the host: an entry outside [0, N) raises IndexError before anything is launched."""
    import ctypes as C
    from . import lib as _lib
    idx = torch.as_tensor(index).reshape(-1).to(device="cpu", dtype=torch.int64)
    N, B, D = int(img_set.shape[0]), int(idx.numel()), int(img_set.shape[-1])
    if B == 0 or int(idx.min()) < 0 or int(idx.max()) >= N:
        raise IndexError(f"gather_windows: index out of range for a set of {N} windows" if B else "gather_windows: empty index")
    for t, dt in ((img_set, torch.float32), (ev_set, torch.float32), (set_lengths, torch.int32)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError("gather_windows: the sets are contiguous fp32 device tensors, their lengths int32")
    if img_set.shape != ev_set.shape or tuple(img_set.shape[1:]) != (_T, D) or set_lengths.numel() != N:
        raise ValueError(f"gather_windows: sets of {tuple(img_set.shape)} / {tuple(ev_set.shape)} windows, {set_lengths.numel()} lengths")
    dev = img_set.device
    # pinned + asynchronous: a pageable copy would make the host wait for everything the stream still holds, every step
    didx = idx.to(torch.int32).pin_memory().to(dev, non_blocking=True)
    img = torch.empty(B, _T, D, dtype=torch.float32, device=dev)
    ev = torch.empty_like(img)
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load_library().iefvad_gather_windows(C.c_void_p(img_set.data_ptr()), C.c_void_p(ev_set.data_ptr()), C.c_void_p(set_lengths.data_ptr()),
                                                       N, C.c_void_p(didx.data_ptr()), B, _T, D, C.c_void_p(img.data_ptr()), C.c_void_p(ev.data_ptr()),
                                                       C.c_void_p(lens.data_ptr()), _stream(dev))
    if rc != 0:
        raise RuntimeError("iefvad_gather_windows: " + _lib.last_error())
    return img, ev, lens


class _RaggedStager:
    """Feature files -> one device tensor of packed rows: the arrays of one dtype are gathered into a reusable pinned buffer by
    `iefvad_host_gather` (a few host threads, no per-file tensor op) and sent with one asynchronous copy on the current stream; a
    buffer is reused only after the event behind its last copy has completed."""

    def __init__(self, device, slots: int = 4):
        self.device = torch.device(device)
        self.threads = max(1, min(8, harness.host_cpu_share() // 2))
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.turn = 0

    def upload(self, arrays: Sequence[np.ndarray]) -> torch.Tensor:
        import ctypes as C
        from . import lib as _lib
        slot = self.turn
        self.turn = (self.turn + 1) % len(self.bufs)
        if self.events[slot] is not None:
            self.events[slot].synchronize()
        arrays = [np.ascontiguousarray(a) for a in arrays]
        dt, D = arrays[0].dtype, int(arrays[0].shape[1])
        nbytes = sum(a.nbytes for a in arrays)
        if self.bufs[slot] is None or self.bufs[slot].numel() < nbytes:
            self.bufs[slot] = torch.empty(max(int(nbytes * 1.25), 1 << 22), dtype=torch.uint8, pin_memory=True)
        tdt = torch.float32 if dt == np.float32 else torch.float16
        host = self.bufs[slot][:nbytes].view(tdt).view(-1, D)
        n = len(arrays)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
        sizes = (C.c_size_t * n)(*[a.nbytes for a in arrays])
        if _lib.load_library().iefvad_host_gather(C.c_void_p(host.data_ptr()), ptrs, sizes, n, self.threads) != 0:
            raise RuntimeError("iefvad_host_gather: " + _lib.last_error())
        dev = host.to(self.device, non_blocking=True)
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(self.device))
        self.events[slot] = e
        return dev


class TrainSetTooLarge(RuntimeError):
    """DeviceTrainSet(resident=True): the windows of the set need more device memory than `budget_bytes`."""


class DeviceTrainSet:
    """A `harness.TrainFeatureDataset` whose windows live on the device.

    resident=True: at construction the files are read in groups whose raw rows fit `staging_bytes` (a larger single video gets an
    upload of its own), staged through pinned memory, uploaded and resampled by `iefvad_resample_videos` into [N, 256, D] fp32
    tensors (`.img`, `.ev`) and int32 `.lengths` (the image file's clip length, dataset.py:52).  A window depends only on its file,
    so this happens once; a step's batch is then `iefvad_gather_windows` by index and no feature row crosses the host link again.
    The set needs N (2 * 256 * D * 4 + 4) bytes; more than `budget_bytes` raises `TrainSetTooLarge` naming that figure.
    resident=False: nothing is kept; every batch stages, uploads and resamples its own videos -- same kernel, same bits.
    Runs of consecutive files of one dtype share a launch; fp32 and fp16 files go in separate launches."""

    def __init__(self, dataset, device, resident: bool = True, staging_bytes: int = 256 << 20, budget_bytes: Optional[int] = None):
        self.dataset = dataset
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceTrainSet resamples on the GPU (csrc/resample.h); there is no CPU fallback for this path -- "
                               "use DataLoader(harness.TrainFeatureDataset) on the host")
        self.resident = bool(resident)
        self.staging_bytes = int(staging_bytes)
        self.labels = list(dataset.labels)
        self._stager = _RaggedStager(self.device, slots=2 if self.resident else 4)
        self.img = self.ev = self.lengths = None
        N = len(dataset)
        if N == 0:
            raise ValueError("DeviceTrainSet: the dataset is empty")
        if dataset.clip_dim != _T:
            raise ValueError(f"DeviceTrainSet: the window is {_T} segments (clip_dim = {dataset.clip_dim})")
        self.D = int(np.load(dataset.paths[0], mmap_mode="r").shape[1])
        self.nbytes = N * (2 * _T * self.D * 4 + 4)
        if self.resident:
            if budget_bytes is not None and self.nbytes > budget_bytes:
                raise TrainSetTooLarge(f"DeviceTrainSet: {N} videos of D = {self.D} need {self.nbytes} bytes on the device, "
                                       f"budget_bytes = {int(budget_bytes)}; use resident=False")
            self._ingest()

    def __len__(self):
        return len(self.labels)

    # one modality of a group of files -> windows written to out[k] (contiguous [len(arrays), 256, D]) and lens[k]
    def _resample_into(self, arrays, out, lens):
        k = 0
        while k < len(arrays):
            j = k
            while j < len(arrays) and arrays[j].dtype == arrays[k].dtype:
                j += 1
            run = arrays[k:j]
            for a in run:
                if a.dtype not in _IN_CODES or a.ndim != 2 or a.shape[1] != self.D or a.shape[0] < 1:
                    raise ValueError(f"DeviceTrainSet: feature files are [n >= 1, {self.D}] fp32 or fp16, got {a.dtype} {a.shape}")
            rows = self._stager.upload(run)
            resample_videos(rows, [a.shape[0] for a in run], out[k:j], lens[k:j])
            k = j

    def _windows_of(self, indices, img_out, ev_out, len_out):
        """Files `indices` -> img_out / ev_out [len(indices), 256, D], len_out int32, in groups bounded by the staging budget."""
        scratch = torch.empty(len(indices), dtype=torch.int32, device=self.device)       # the event files' own clip lengths: not carried
        g0, imgs, evs, held = 0, [], [], 0

        def flush(g1):
            self._resample_into(imgs, img_out[g0:g1], len_out[g0:g1])
            self._resample_into(evs, ev_out[g0:g1], scratch[g0:g1])

        for pos, i in enumerate(indices):
            img, ev = self.dataset.load_raw(int(i))
            if imgs and held + img.nbytes + ev.nbytes > self.staging_bytes:
                flush(pos)
                g0, imgs, evs, held = pos, [], [], 0
            imgs.append(img)
            evs.append(ev)
            held += img.nbytes + ev.nbytes
        flush(len(indices))

    def _ingest(self):
        N = len(self)
        self.img = torch.empty(N, _T, self.D, dtype=torch.float32, device=self.device)
        self.ev = torch.empty_like(self.img)
        self.lengths = torch.empty(N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._windows_of(range(N), self.img, self.ev, self.lengths)
            torch.cuda.current_stream(self.device).synchronize()
        self._stager = None                       # its pinned buffers are not needed again: batches come from the cached windows

    def batch(self, index):
        """(img [B, 256, D], ev [B, 256, D], labels list[str], lengths int32 [B]) for the videos `index`: fresh device tensors, so the
        trainers' in-place NaN repair (`_nan_rule_pair`) never reaches the cached set."""
        index = torch.as_tensor(index).reshape(-1).to(device="cpu", dtype=torch.int64)
        with torch.cuda.device(self.device):
            if self.resident:
                img, ev, lens = gather_windows(self.img, self.ev, self.lengths, index)      # checks the range, on the host
                labels = [self.labels[i] for i in index.tolist()]
            else:
                idx = index.tolist()
                if not idx or min(idx) < 0 or max(idx) >= len(self):
                    raise IndexError(f"DeviceTrainSet: index out of range for a set of {len(self)} videos")
                labels = [self.labels[i] for i in idx]
                img = torch.empty(len(idx), _T, self.D, dtype=torch.float32, device=self.device)
                ev = torch.empty_like(img)
                lens = torch.empty(len(idx), dtype=torch.int32, device=self.device)
                self._windows_of(idx, img, ev, lens)
        return img, ev, labels, lens

    def loader(self, batch_size: int, shuffle: bool = True, drop_last: bool = False):
        return DeviceTrainLoader(self, batch_size, shuffle, drop_last)


class DeviceTrainLoader:
    """What `train_paired` / `train_single` iterate: `__len__`, `__iter__`, `.batch_size`.  The sampling order comes from a
    `torch.utils.data.DataLoader` over the INDICES with the same arguments, so under one `torch.manual_seed` the batches are exactly
    those of `DataLoader(TrainFeatureDataset, batch_size, shuffle, drop_last)` -- already on the device."""

    def __init__(self, trainset: DeviceTrainSet, batch_size: int, shuffle: bool, drop_last: bool):
        self.trainset = trainset
        self.batch_size = batch_size
        self._indices = torch.utils.data.DataLoader(list(range(len(trainset))), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last)

    def __len__(self):
        return len(self._indices)

    def __iter__(self):
        it = iter(self._indices)              # NOW, as DataLoader.__iter__ does: the epoch's seeds leave torch's generator at this call,
                                              # not at the first next() (train_paired opens both loaders before it reads either)
        return (self.trainset.batch(idx) for idx in it)


def get_device_train_loaders(args, device, dataset: Optional[str] = None, **kw):
    """`harness.get_train_loaders` with the sets on the device: (normal_loader, abnormal_loader) for ucfcrime / shang / msad, one loader
    for xd, the same sampling arguments.  `kw` goes to `DeviceTrainSet` (resident, staging_bytes, budget_bytes)."""
    dataset = dataset or args.dataset
    if dataset == 'xd':
        return DeviceTrainSet(harness.TrainFeatureDataset(args.visual_length, args.train_list, 'xd'), device, **kw).loader(args.batch_size, True, False)
    return tuple(DeviceTrainSet(harness.TrainFeatureDataset(args.visual_length, args.train_list, dataset, normal=flag), device, **kw)
                 .loader(args.batch_size, True, True) for flag in (True, False))
