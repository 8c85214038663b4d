"""Data-parallel inference over the GPUs of one node: one process per GPU, ``torch.distributed``
(backend ``nccl`` = RCCL over xGMI on ROCm; ``gloo`` on CPU for the tests).

The reference has no multi-GPU inference; images are independent end to end
(pipeline.py:62-75), so the batch is split into contiguous blocks, each rank runs the whole
detect -> crop -> recognise chain on its block, and only the results (a few kB per image: boxes
+ strings) cross ranks.  The one cross-image coupling — ``pad`` to the batch's maximum size
(pipeline.py:48-57) — is resolved BEFORE sharding so that every rank sees the same detector
input size as the single-process call would.  No all-reduce, no data-path collective.
"""
import os

import numpy as np


# The width of a label row is the recogniser's: 50 time-steps minus its rnn_steps_to_discard (recognition.py:175-182, 328; 48
# for the default build).  Nothing here assumes a value: a rank reads the width off its own label rows, or asks its recogniser
# when it has none, and the ranks compare what they read in the counts exchange (the status slot's upper bits).
_STATUS_BITS = 8  # the status slot: the exception code in the low byte, the rank's label width (0 = no opinion) above it


def init_from_env(backend=None, force=False):
    """Initialise torch.distributed from RANK / WORLD_SIZE / MASTER_* (torchrun's contract).
    ``force`` creates the process group even for a single rank, so that the RCCL path is the one that
    runs (and is exercised) at N = 1 too."""
    import torch
    import torch.distributed as dist

    if dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and not force:
        return 0, 1
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver
    if backend == "nccl":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dist.init_process_group(backend=backend)
    return dist.get_rank(), dist.get_world_size()


def shard_bounds(n_items, world_size, rank):
    """Contiguous block [start, end) of ceil(n/world) items for ``rank``."""
    per = -(-n_items // world_size) if n_items else 0
    start = min(rank * per, n_items)
    return start, min(start + per, n_items)


def _comm_device(group=None):
    """Tensors handed to a collective live where the backend wants them: HBM for nccl (= RCCL), host for gloo."""
    import torch
    import torch.distributed as dist

    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")


def ranks_seen(group=None):
    """All-reduce of 1 over the group: the number of ranks that really took part (1 without a group)."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return 1
    one = torch.ones(1, dtype=torch.int32, device=_comm_device(group))
    dist.all_reduce(one, op=dist.ReduceOp.SUM, group=group)
    return int(one.item())


def packed_payload_bytes(per_rank_images, cap, label_width=48):
    """Bytes ONE rank contributes to the three all-gathers of `gather_packed` (counts, boxes, label rows of ``label_width``
    columns: 48 for the default recogniser build).  The width itself travels in the status slot of the counts: no bytes."""
    cap, label_width = max(int(cap), 1), int(label_width)
    return {"counts": 4 * (per_rank_images + 2), "boxes": cap * 8 * 4, "labels": cap * label_width * 4,
            "total": 4 * (per_rank_images + 2) + cap * 8 * 4 + cap * label_width * 4}


class ShardError(RuntimeError):
    """Raised on EVERY rank when the local chain of at least one rank failed.  The message names the failing rank(s) and
    the KIND of exception each raised (exchanged as a small code in the status slot of the counts all-gather: the
    reference's IndexError at detection.py:272 / ZeroDivisionError at tools.py:95, an AssertionError, a libkocr error, or
    "Exception"), also available as ``failed_ranks`` / ``kinds`` ({rank: name}); the failing rank chains its own
    exception as ``__cause__``.  A sharded caller therefore sees ShardError where the single-process call raises the
    reference's own exception type."""
    failed_ranks = ()
    kinds = {}


_STATUS_NAMES = {1: "Exception", 2: "IndexError", 3: "ZeroDivisionError", 4: "AssertionError", 5: "KocrError", 6: "ValueError",
                 7: "TypeError"}


def _status_of(error):
    """0 = ok, else a code naming the exception type (anything unlisted travels as 1 = "Exception")."""
    if error is None:
        return 0
    for code, name in _STATUS_NAMES.items():
        if code != 1 and any(c.__name__ == name for c in type(error).__mro__):
            return code
    return 1


class _DeviceArray:
    """A device buffer libkocr owns, as something ``torch.as_tensor(..., device="cuda")`` takes without a copy."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def _pack_tensors(counts, boxes, labels, cap, dev, label_width=None):
    """(cap, 8) box tensor and (cap, label width) label tensor from the per-image form kocr_pipeline produces -- counts [n],
    boxes [n][cap_local][8] (rows >= counts[i] of image i undefined), label rows [m][label width] -- on whatever device the
    inputs live: a boolean-mask gather by the counts, image-major, which is the order of the label rows.  The width is the
    rows' own; ``label_width`` says it for a rank without rows (``labels`` None; 48, the default build's, when it is None too)
    and must agree with rows that are there."""
    import torch

    n, cl = boxes.shape[0], boxes.shape[1]
    m = int(labels.shape[0]) if labels is not None else 0
    if labels is not None and label_width is not None and int(labels.shape[1]) != int(label_width):
        raise ValueError(f"_pack_tensors: label rows of width {int(labels.shape[1])} packed as width {int(label_width)}")
    # no rows and nobody to say the width: the default build's, as gather_packed does when no rank has an opinion
    lw = int(labels.shape[1]) if labels is not None else 48 if label_width is None else int(label_width)
    b = torch.zeros((cap, 8), dtype=torch.float32, device=dev)
    l = torch.full((cap, lw), -1, dtype=torch.int32, device=dev)
    if m:
        mask = torch.arange(cl, device=dev)[None, :] < counts[:, None]
        b[:m] = boxes.reshape(n, cl, 8)[mask]
        l[:m] = labels
    return b, l


def _pack_on_device(dev_res, cap, dev, label_width):
    """The packed tensors of gather_packed built IN HBM from what kocr_pipeline left there: the payload RCCL moves never
    visits the host.  The device rows are viewed at the width they were produced with (``dev_res["lw"]``), which must be the
    width the ranks agreed on (``label_width``)."""
    import torch

    n, cl, m, lw = dev_res["n"], dev_res["cap"], dev_res["m"], dev_res["lw"]
    if m and lw != label_width:
        raise ValueError(f"_pack_on_device: resident label rows of width {lw}, the gather runs at {label_width}")
    counts = torch.as_tensor(_DeviceArray(dev_res["counts"], (n,), "<i4"), device=dev)
    boxes = torch.as_tensor(_DeviceArray(dev_res["boxes"], (n, cl, 8), "<f4"), device=dev)
    labels = torch.as_tensor(_DeviceArray(dev_res["labels"], (m, lw), "<i4"), device=dev) if m else None
    return _pack_tensors(counts, boxes, labels, cap, dev, label_width)


def _label_rows(labels, m):
    """``labels`` as an (m, width) int32 array; ValueError for anything that is not m rows of one width"""
    labels = np.asarray(labels, np.int32)
    if not m and not labels.size:
        return np.zeros((0, labels.shape[1] if labels.ndim == 2 else 0), np.int32)
    if labels.ndim != 2 and m and labels.size and labels.size % m == 0:
        labels = labels.reshape(m, -1)
    if labels.ndim != 2 or labels.shape[0] != m or (m and not labels.shape[1]):
        raise ValueError(f"label rows of shape {labels.shape} for {m} boxes")
    return labels


def gather_packed(box_groups, labels, per_rank_images, group=None, error=None, timing=None, device_results=None,
                  device_scale=None, label_width=None):
    """all-gather of the per-image box counts, then of fixed-capacity packed results.

    Every rank contributes ``per_rank_images`` count slots (its shard, zero padded), a (cap, 8) float32
    box tensor and a (cap, label width) int32 label tensor, where cap = the largest crop count of any rank (known
    after the counts exchange).  Three collectives, no pickling; on the nccl backend the tensors stay in
    HBM and travel over xGMI.  Returns (box_groups, labels) of the whole batch in image order.

    The label width (48 by default: 50 - the recogniser's rnn_steps_to_discard) is never assumed.  A rank with rows takes
    the width of its rows; a rank without rows says ``label_width`` (its recogniser's: ``ShardedPipeline`` passes it), else
    the width of its zero-row array, and has no opinion (0) when that is 0 too.  The widths travel in the upper bits of the
    status slot of the counts exchange, so no collective and no byte is added: ranks without an opinion adopt the others'
    width and enter the label gather with a (cap, width) tensor of -1; two different widths raise ``ShardError`` naming the
    ranks on EVERY rank, after the first collective like any failure; when no rank has an opinion there are no rows
    either, and the result is (0, 48).

    ``device_scale`` (nccl backend, the SAME value on every rank or None on every rank) switches the box / label gathers to
    device-originated payloads: a rank that had work passes ``device_results`` (``Pipeline.recognize_device_raw``: where its
    results still lie in HBM, boxes in detector-input pixels) and its packed tensors are built on the device from those
    buffers (`_pack_on_device`) -- nothing is copied up from the host; every rank then divides the gathered boxes by the
    scale exactly as the host path does before its gather (``tools.adjust_boxes``: the same float32 product), so the result
    is identical bit for bit.

    ``error``: the exception the local chain raised, if any.  The counts exchange carries a status slot, so a
    data-dependent failure on one rank (the reference raises IndexError at detection.py:272 on an empty contour
    list, ZeroDivisionError at tools.py:95) makes EVERY rank raise ``ShardError`` after the first collective instead
    of leaving the others blocked in the box / label gathers.  ``timing`` (a dict) receives ``gather_s``.
    """
    import time
    import torch
    import torch.distributed as dist

    opinion = int(label_width or 0)
    if error is not None:
        box_groups, labels = [], np.zeros((0, opinion), np.int32)
    counts_local = [len(b) for b in box_groups]
    m_local = int(sum(counts_local))
    labels = _label_rows(labels, m_local)
    lw_local = int(labels.shape[1]) if m_local else (opinion or int(labels.shape[1]))
    boxes_local = (np.concatenate([np.asarray(b, np.float32).reshape(-1, 8) for b in box_groups if len(b)])
                   if m_local else np.zeros((0, 8), np.float32))
    if not (dist.is_available() and dist.is_initialized()):
        if error is not None:
            raise error
        return [np.asarray(b) for b in box_groups], labels
    t0 = time.perf_counter()
    world = dist.get_world_size(group)
    dev = _comm_device(group)
    if error is None and device_scale is not None and dev.type == "cuda" and m_local and \
            (not device_results or device_results.get("m") != m_local):
        # found BEFORE the first collective and sent through the status slot: raised locally after the counts exchange it would
        # leave the other ranks blocked in the box / label gathers
        error = RuntimeError("gather_packed: device-originated gather without this rank's device results")
        box_groups, labels = [], np.zeros((0, lw_local), np.int32)
        counts_local, m_local, boxes_local = [], 0, np.zeros((0, 8), np.float32)
    if error is None and device_scale is not None and dev.type == "cuda" and m_local and device_results.get("lw") != lw_local:
        # likewise: rows that lie in HBM at another pitch than the host rows say are not viewed at all
        error = RuntimeError(f"gather_packed: the resident label rows have width {device_results.get('lw')}, the host rows {lw_local}")
        box_groups, labels = [], np.zeros((0, lw_local), np.int32)
        counts_local, m_local, boxes_local = [], 0, np.zeros((0, 8), np.float32)
    # 1. counts: per_rank_images + 2 ints per rank (slot -2 = number of images this rank really had, slot -1 = status in the
    # low byte, this rank's label width above it)
    c = torch.zeros(per_rank_images + 2, dtype=torch.int32)
    c[:len(counts_local)] = torch.tensor(counts_local, dtype=torch.int32)
    c[-2] = len(counts_local)
    c[-1] = _status_of(error) | (lw_local << _STATUS_BITS)
    c = c.to(dev)
    all_c = torch.empty(world * (per_rank_images + 2), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(all_c, c, group=group)
    all_c = all_c.cpu().numpy().reshape(world, per_rank_images + 2)
    status = all_c[:, -1] & ((1 << _STATUS_BITS) - 1)
    widths = all_c[:, -1] >> _STATUS_BITS
    failed = [r for r in range(world) if status[r] != 0]
    if failed:
        kinds = sorted({_STATUS_NAMES.get(int(status[r]), "Exception") for r in failed})
        msg = f"sharded recognize failed on rank(s) {failed} ({', '.join(kinds)})"
        exc = ShardError(f"{msg}: {type(error).__name__}: {error}" if error is not None else msg)
        exc.failed_ranks = failed
        exc.kinds = {r: _STATUS_NAMES.get(int(status[r]), "Exception") for r in failed}
        if error is not None:
            raise exc from error
        raise exc
    said = {r: int(widths[r]) for r in range(world) if widths[r] != 0}
    if len(set(said.values())) > 1:
        # every rank sees the same widths and raises here, before the box / label gathers: nobody is left in a collective
        exc = ShardError(f"sharded recognize failed on rank(s) {sorted(said)} (LabelWidth): the ranks disagree on the label width "
                         f"{said} ({{rank: width}}; every recogniser must be built with the same rnn_steps_to_discard)")
        exc.failed_ranks = sorted(said)
        exc.kinds = {r: "LabelWidth" for r in said}
        raise exc
    lw = next(iter(said.values())) if said else 48  # nobody has rows or a recogniser to ask: the default build's empty result
    cap = max(int(all_c[:, :-2].sum(axis=1).max()), 1)
    # 2. + 3. packed boxes and label rows, capacity = the busiest rank's crop count
    # every rank must take the same branch below: the scale travels with the decision (all ranks of a device-resident batch
    # have it or none has: recognize_device / recognize_scattered pass it on every rank that had work)
    on_device = device_scale is not None and dev.type == "cuda"
    if on_device and m_local:
        b, l = _pack_on_device(device_results, cap, dev, lw)
    elif on_device:
        b = torch.zeros((cap, 8), dtype=torch.float32, device=dev)
        l = torch.full((cap, lw), -1, dtype=torch.int32, device=dev)
    else:
        b = torch.zeros((cap, 8), dtype=torch.float32)
        b[:m_local] = torch.from_numpy(boxes_local)
        l = torch.full((cap, lw), -1, dtype=torch.int32)
        if m_local:
            l[:m_local] = torch.from_numpy(labels)
        b, l = b.to(dev), l.to(dev)
    all_b = torch.empty((world * cap, 8), dtype=torch.float32, device=dev)
    all_l = torch.empty((world * cap, lw), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(all_b, b, group=group)
    dist.all_gather_into_tensor(all_l, l, group=group)
    all_b = all_b.cpu().numpy().reshape(world, cap, 4, 2)
    all_l = all_l.cpu().numpy().reshape(world, cap, lw)
    if on_device and device_scale != 1:
        all_b = all_b * (1 / device_scale)  # tools.adjust_boxes (pipeline.py:66-71), as Pipeline._adjust does on the host path
    if timing is not None:
        timing["gather_packed_on_device"] = on_device
    if timing is not None:
        timing["gather_s"] = timing.get("gather_s", 0.0) + (time.perf_counter() - t0)
        timing["gather_payload_bytes_per_rank"] = packed_payload_bytes(per_rank_images, cap, lw)["total"]
    out_boxes, out_labels = [], []
    for r in range(world):
        pos = 0
        for i in range(int(all_c[r, -2])):
            n = int(all_c[r, i])
            # an image without boxes is np.array([]) in the reference (detection.py:286)
            out_boxes.append(all_b[r, pos:pos + n].copy() if n else np.zeros((0,), np.float32))
            pos += n
        out_labels.append(all_l[r, :pos])
    return out_boxes, np.concatenate(out_labels) if out_labels else np.zeros((0, lw), np.int32)


class ShardedPipeline:
    """``Pipeline.recognize`` over all ranks: same arguments, same return value on every rank."""

    def __init__(self, pipeline, group=None):
        self.pipeline = pipeline
        self.group = group

    def _rank_world(self):
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(self.group), dist.get_world_size(self.group)
        return 0, 1

    @staticmethod
    def _refuse_scores(return_scores):
        if return_scores:
            raise NotImplementedError("ShardedPipeline does not carry scores across ranks: its packed result rows hold boxes and "
                                      "labels only; use Pipeline.recognize(..., return_scores=True) on each rank's own pages")

    @staticmethod
    def _refuse_beam(recognition_kwargs):
        if (recognition_kwargs or {}).get("beam_width") is not None:
            raise NotImplementedError("ShardedPipeline does not carry beam alternatives across ranks: its packed result rows hold "
                                      "boxes and one label row per word; use Pipeline.recognize(..., recognition_kwargs="
                                      "{'beam_width': ...}) on each rank's own pages")

    @staticmethod
    def _refuse_lexicon(recognition_kwargs):
        if (recognition_kwargs or {}).get("lexicon_top") is not None:
            raise NotImplementedError("ShardedPipeline does not carry lexicon matches across ranks: its packed result rows hold "
                                      "boxes and one label row per word; use Pipeline.recognize(..., recognition_kwargs="
                                      "{'lexicon_top': ...}) on each rank's own pages")

    @staticmethod
    def _refuse_orientation(recognition_kwargs):
        if (recognition_kwargs or {}).get("orientation") is not None:
            raise NotImplementedError("ShardedPipeline does not carry orientation across ranks: its packed result rows hold "
                                      "getBoxes' boxes and one label row per word; use Pipeline.recognize(..., recognition_kwargs="
                                      "{'orientation': ...}) on each rank's own pages")

    @staticmethod
    def _refuse_pattern(recognition_kwargs):
        if (recognition_kwargs or {}).get("pattern") is not None:
            raise NotImplementedError("ShardedPipeline does not carry pattern decodes across ranks: its packed result rows hold "
                                      "boxes and one label row per word; use Pipeline.recognize(..., recognition_kwargs="
                                      "{'pattern': ...}) on each rank's own pages")

    def recognize(self, images, detection_kwargs=None, recognition_kwargs=None, timing=None, return_scores=False):
        """``timing`` (optional dict) receives ``gather_s``: the time spent in the three result all-gathers.
        ``return_scores=True`` and a ``beam_width``, ``lexicon_top``, ``orientation`` or ``pattern`` in ``recognition_kwargs``
        are refused (NotImplementedError): neither scores nor beam alternatives nor lexicon matches nor orientation nor
        pattern decodes cross ranks."""
        from . import tools

        self._refuse_scores(return_scores)
        self._refuse_beam(recognition_kwargs)
        self._refuse_lexicon(recognition_kwargs)
        self._refuse_orientation(recognition_kwargs)
        self._refuse_pattern(recognition_kwargs)

        if not isinstance(images, np.ndarray):
            images = [tools.read(image) for image in images]
        images = list(images)
        if not images:
            return []
        rank, world = self._rank_world()
        # the padded size comes from the WHOLE batch (pipeline.py:48-57), not from the shard
        _, _, _, hmax, wmax = self.pipeline._plan([im.shape for im in images])  # pylint: disable=protected-access
        start, end = shard_bounds(len(images), world, rank)
        return self._run_shard(lambda: self.pipeline.recognize_raw(images[start:end], hmax, wmax, detection_kwargs,
                                                                   recognition_kwargs),
                               end > start, -(-len(images) // world), timing)

    def recognize_device(self, d_ptr, n_total, h, w, detection_kwargs=None, timing=None, return_scores=False):
        """The same for a batch whose images are already resident in THIS rank's HBM (``d_ptr`` = device pointer of this
        rank's contiguous block of images of the (n_total, h, w, 3) uint8 batch): every image has the same size, so the
        whole batch's padded size is the shard's.  ``return_scores=True`` is refused as in ``recognize``."""
        self._refuse_scores(return_scores)
        rank, world = self._rank_world()
        start, end = shard_bounds(n_total, world, rank)
        dev_res, scale = self._device_gather(n_total, h, w)
        return self._run_shard(lambda: self.pipeline.recognize_device_raw(d_ptr, end - start, h, w, detection_kwargs, *(() if dev_res is None else (dev_res,))),
                               end > start, -(-n_total // world), timing, dev_res, scale)

    def _device_gather(self, n_total, h, w):
        """(dict to receive the device results, scale) when the result gathers can be device-originated -- RCCL group, the
        real Pipeline (one image size, hence one scale, known on every rank from the plan) -- else (None, None)."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized() and dist.get_backend(self.group) == "nccl" and n_total > 0 and
                hasattr(self.pipeline, "recognize_device_raw") and getattr(getattr(self.pipeline, "detector", None), "_ctx", None) is not None):
            return None, None
        scales = self.pipeline._plan([(h, w, 3)] * n_total)[0]  # pylint: disable=protected-access
        return {}, scales[0]

    def recognize_scattered(self, batch, n_total, h, w, src_rank=0, detection_kwargs=None, timing=None):
        """the WHOLE (n_total, h, w, 3) uint8 batch starts on ONE rank -- ``batch`` is a torch tensor
        in ``src_rank``'s HBM (a host tensor under gloo) and is ignored (may be None) on the other ranks.  The raw pages
        are scattered BEFORE the resize (the smallest form of the data: 1.81 GB for BASELINE configs[4], 7/8 of it leaves
        rank 0 over its seven xGMI links) with one ``torch.distributed.scatter`` of equal ceil(n/world) blocks (RCCL
        implements it as grouped send/recv; the last block is zero padded), then every rank runs the local chain on its
        block and the results are all-gathered as in ``recognize_device``.  ``timing`` receives ``scatter_s`` (the
        collective plus the wait for it) and ``scatter_bytes_sent`` next to ``gather_s``."""
        import time
        import torch
        import torch.distributed as dist

        rank, world = self._rank_world()
        per = -(-n_total // world) if n_total else 0
        start, end = shard_bounds(n_total, world, rank)
        distributed = dist.is_available() and dist.is_initialized()
        t0 = time.perf_counter()
        src_error = None
        if not distributed:
            mine = batch
            dev = None
        else:
            dev = _comm_device(self.group)
            # The source rank may fail BEFORE the collective (a missing / mis-shaped batch, an allocation error while it
            # cuts the blocks): every other rank would already sit in the scatter and hang until the backend's timeout.
            # So the source first tells everybody whether the scatter will happen (one int32 broadcast); on failure no
            # rank enters it, and the error travels through the status slot of the counts all-gather like any failure of a
            # local chain: ShardError on every rank.
            chunks = None
            if rank == src_rank:
                try:
                    if batch is None or tuple(batch.shape) != (n_total, h, w, 3) or batch.dtype != torch.uint8:
                        raise ValueError("recognize_scattered: the source rank needs the (n_total, h, w, 3) uint8 batch")
                    batch = batch.to(dev)
                    chunks = []
                    for r in range(world):
                        c = batch[r * per:min((r + 1) * per, n_total)]
                        if c.shape[0] < per:  # equal blocks for the collective: the tail is zero padded (and never processed)
                            c = torch.cat([c, torch.zeros((per - c.shape[0], h, w, 3), dtype=torch.uint8, device=dev)])
                        chunks.append(c.contiguous())
                except Exception as e:  # noqa: BLE001 -- exchanged below, never raised on this rank alone
                    src_error, chunks = e, None
            go = torch.tensor([0 if src_error is not None else 1], dtype=torch.int32, device=dev)
            dist.broadcast(go, src=src_rank, group=self.group)
            mine = None
            if int(go.item()) == 1:
                mine = torch.empty((per, h, w, 3), dtype=torch.uint8, device=dev)
                dist.scatter(mine, scatter_list=chunks, src=src_rank, group=self.group)
                if dev.type == "cuda":
                    torch.cuda.synchronize()
        if timing is not None:
            timing["scatter_s"] = timing.get("scatter_s", 0.0) + (time.perf_counter() - t0)
            timing["scatter_bytes_sent"] = (per * (world - 1) * h * w * 3) if (distributed and rank == src_rank and src_error is None) else 0
        n_mine = end - start

        dev_res, scale = self._device_gather(n_total, h, w)

        def run():
            if src_error is not None:
                raise src_error
            if mine.device.type == "cuda":
                return self.pipeline.recognize_device_raw(mine.data_ptr(), n_mine, h, w, detection_kwargs, *(() if dev_res is None else (dev_res,)))
            # host tensors (gloo): the same call as recognize(); every image has the batch's size
            _, _, _, hmax, wmax = self.pipeline._plan([(h, w, 3)] * n_total)  # pylint: disable=protected-access
            return self.pipeline.recognize_raw(mine[:n_mine].numpy(), hmax, wmax, detection_kwargs, None)

        if distributed and mine is None:  # the source failed: nobody has a block; the source reports why
            return self._run_shard(run, rank == src_rank, per, timing, dev_res, scale)
        return self._run_shard(run, n_mine > 0, per, timing, dev_res, scale)

    def _label_width(self):
        """The width of the recogniser's label rows -- its libkocr context's ``crnn_label_width()``, else its ``label_width``
        attribute -- for a rank that has no rows to read it off; 0 (no opinion) for a recogniser that says neither."""
        from .pipeline import label_width_of

        return label_width_of(getattr(self.pipeline, "recognizer", self.pipeline)) or 0

    def _run_shard(self, run, has_work, per, timing, device_results=None, device_scale=None):
        box_groups, labels, err, lw = [], None, None, 0
        try:
            lw = self._label_width()
            labels = np.zeros((0, lw), np.int32)
            if has_work:
                box_groups, labels = run()
                # the packing of gather_packed's preamble, done here so that a malformed local result is exchanged as a
                # status too instead of raising on one rank before the first collective
                labels = _label_rows(labels, sum(len(b) for b in box_groups))
                for b in box_groups:
                    if len(b):
                        np.asarray(b, np.float32).reshape(-1, 8)
        except Exception as e:  # noqa: BLE001 -- exchanged as a status flag so that no rank is left in a collective
            box_groups, labels, err = [], np.zeros((0, lw), np.int32), e
        box_groups, labels = gather_packed(box_groups, labels, per, self.group, error=err, timing=timing,
                                           device_results=device_results, device_scale=device_scale, label_width=lw)
        return self.pipeline.assemble(box_groups, labels)
