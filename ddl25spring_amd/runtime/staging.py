"""Host values to the device without a blocking copy: a pinned stager and a bounded table cache."""
import numpy as np
import torch


class PinnedStager:
    """Two pinned host buffers of ``shape``, used alternately: the copy out of one is truly
    asynchronous, and the host refills it only after the event recorded behind that copy, so with
    ``FederatedBase.sync_rounds`` off it prepares round r+1 while the GPU still runs round r."""

    def __init__(self, shape, dtype: torch.dtype):
        self.shape, self.dtype = tuple(shape), dtype
        self._slots = None  # [[pinned buffer, event of its last copy]] * 2, from the first GPU use
        self._cur = 0

    def put(self, values: np.ndarray, dst):
        """values (``shape``, or shorter along the first axis) -> ``dst``: a device tensor of the
        values' shape, or a ``torch.device`` for a fresh one. On a CPU device a plain copy."""
        fresh = isinstance(dst, torch.device)
        dev = dst if fresh else dst.device
        if dev.type != "cuda":
            src = torch.from_numpy(values)
            return src.to(dev) if fresh else dst.copy_(src)
        if self._slots is None:
            self._slots = [[torch.empty(self.shape, dtype=self.dtype, pin_memory=True), None] for _ in range(2)]
        self._cur ^= 1
        slot = self._slots[self._cur]
        if slot[1] is not None:
            slot[1].synchronize()  # the copy that last read this buffer (two uses ago) is done
        src = slot[0][:len(values)]
        src.numpy()[...] = values
        out = src.to(dev, non_blocking=True) if fresh else dst.copy_(src, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return out


class DeviceTables:
    """Device tensors built from host lists, cached by key: building one is a blocking copy. At most
    ``cap`` are kept; beyond that ``get`` returns a fresh tensor and stores nothing."""

    def __init__(self, cap: int = 256):
        self.cap, self._tables = cap, {}

    def __len__(self) -> int:
        return len(self._tables)

    def get(self, key, build):
        t = self._tables.get(key)
        if t is None:
            t = build()
            if len(self._tables) < self.cap:
                self._tables[key] = t
        return t
