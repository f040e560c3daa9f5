"""The logger DiffusionBC writes to (reference: offlinerlkit/utils/diffusion_logger.py, a stable-baselines3 style logger): the three
methods the policy calls -- ``record``, ``record_mean``, ``dump`` -- and ``dir``, where the checkpoints go.  ``utils.logger.Logger`` has
none of the three (its interface is logkv / dumpkvs), hence this minimal counterpart: one ``progress.csv`` row per ``dump``."""
from __future__ import annotations

import csv
import os
from typing import Any, Dict, Optional


class Logger:
    def __init__(self, folder: Optional[str], output_formats=None) -> None:
        self.dir = folder
        self.name_to_value: Dict[str, Any] = {}
        self.name_to_count: Dict[str, int] = {}
        self._keys = None
        if folder is not None:
            os.makedirs(folder, exist_ok=True)

    def record(self, key: str, value: Any, exclude=None) -> None:
        self.name_to_value[key] = value

    def record_mean(self, key: str, value: Any, exclude=None) -> None:
        if value is None:
            return
        n = self.name_to_count.get(key, 0)
        self.name_to_value[key] = (self.name_to_value.get(key, 0.0) * n + value) / (n + 1)
        self.name_to_count[key] = n + 1

    def dump(self, step: int = 0) -> None:
        row = dict(self.name_to_value, step=step)
        if self.dir is not None:
            path = os.path.join(self.dir, "progress.csv")
            if self._keys is None:
                self._keys = sorted(row)
                with open(path, "w", newline="") as fh:
                    csv.writer(fh).writerow(self._keys)
            with open(path, "a", newline="") as fh:
                csv.writer(fh).writerow([row.get(k, "") for k in self._keys])
        self.name_to_value.clear()
        self.name_to_count.clear()

    def get_dir(self) -> Optional[str]:
        return self.dir
