"""LeRobot v3.0 on-disk I/O of the expert datasets: the episode record, the streaming writer, the
reader and the shard merge.  Host only (numpy + pyarrow, no torch); the episodes come from
`dataset.collect_episodes`, which runs them on the GPU.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass, field

import numpy as np

from .constants import BINS, CONTROL_FPS, IMAGE_SIZE, OBJECTS

# features.py:10-106 (IMAGE_SIZE = 224)
FEATURES = {
    "observation.images.overhead": {"dtype": "image", "shape": (224, 224, 3), "names": ["height", "width", "channels"]},
    "observation.images.wrist": {"dtype": "image", "shape": (224, 224, 3), "names": ["height", "width", "channels"]},
    "observation.state": {"dtype": "float32", "shape": (11,), "names": None},
    "observation.state.ee.pos_quat_g": {"dtype": "float32", "shape": (8,), "names": None},
    "observation.state.ee.pos_rot6d_g": {"dtype": "float32", "shape": (10,), "names": None},
    "observation.state.ee.pos_quat_g_rel": {"dtype": "float32", "shape": (8,), "names": None},
    "observation.state.ee.pos_rot6d_g_rel": {"dtype": "float32", "shape": (10,), "names": None},
    "action.ee.pos_quat_g": {"dtype": "float32", "shape": (8,), "names": None},
    "action.ee.pos_rot6d_g": {"dtype": "float32", "shape": (10,), "names": None},
    "action.ee.pos_quat_g_rel": {"dtype": "float32", "shape": (8,), "names": None},
    "action.ee.pos_rot6d_g_rel": {"dtype": "float32", "shape": (10,), "names": None},
    "observation.target_bin_onehot": {"dtype": "float32", "shape": (3,), "names": None},
    "observation.target_obj_onehot": {"dtype": "float32", "shape": (3,), "names": None},
    "observation.keypoints_overhead": {"dtype": "float32", "shape": (14,), "names": None},
    "observation.keypoints_wrist": {"dtype": "float32", "shape": (14,), "names": None},
    "observation.target_obj_keypoints_overhead": {"dtype": "float32", "shape": (2,), "names": None},
    "observation.target_bin_keypoints_overhead": {"dtype": "float32", "shape": (2,), "names": None},
    "observation.phase_description": {"dtype": "string", "shape": (1,), "names": None},
    "next.reward": {"dtype": "float32", "shape": (6,), "names": None},
}


def make_task_string(obj_name: str, bin_name: str) -> str:
    """generate_dataset.py:41-54."""
    return f"Pick {obj_name.replace('obj_', '')} object and place in {bin_name.replace('bin_', '')} bin"


def resolve_features(features=None, reward_type="staged"):
    """generate_dataset.py:218-230: subset selection, unknown keys -> ValueError,
    next.reward only with the staged reward."""
    feats = dict(FEATURES)
    if features is not None:
        requested = list(features)
        unknown = [k for k in requested if k not in FEATURES]
        if unknown:
            raise ValueError(f"Unknown feature keys: {unknown}. Valid keys: {list(FEATURES.keys())}")
        feats = {k: FEATURES[k] for k in requested}
    if reward_type != "staged":
        feats.pop("next.reward", None)
    return feats


def _features_at(feats: dict, image_size: int) -> dict:
    """The feature schema with the image features at the rendered size (features.py:11-20 states
    224 x 224; the renderer takes any size)."""
    return {k: (dict(v, shape=(image_size, image_size, 3)) if v["dtype"] == "image" else v) for k, v in feats.items()}


@dataclass
class Episode:
    index: int
    obj: str
    bin: str
    seed: int | None
    frames: dict = field(default_factory=dict)  # feature -> np.ndarray [T, ...] (strings, PNG bytes: list)
    length: int = 0
    image_stats: dict = field(default_factory=dict)  # image feature -> stats of a raw frame sample


class PngFrames:
    """An episode's PNG files back to back in one uint8 buffer (file i = data[offsets[i]:offsets[i+1]]).
    Reads as a sequence of `bytes` (len, indexing, iteration) wherever a list of PNG files is expected;
    the LeRobot writer hands the buffer to arrow as is (no Python object per frame)."""
    __slots__ = ("data", "offsets")

    def __init__(self, data: np.ndarray, offsets: np.ndarray):
        self.data, self.offsets = data, offsets

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return self.data[int(self.offsets[i]):int(self.offsets[i + 1])].tobytes()

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def nbytes(self) -> int:
        return int(self.offsets[-1])


def _png_nbytes(frames) -> int:
    return frames.nbytes if isinstance(frames, PngFrames) else sum(map(len, frames))


def png_encode(img: np.ndarray) -> bytes:
    """uint8 [H, W, 3] -> PNG bytes (what LeRobot embeds for an `image` feature)."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(buf, format="PNG", compress_level=1)
    return buf.getvalue()


def png_decode(data: bytes) -> np.ndarray:
    import io

    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _raw_image_stats(frames_u8: list) -> dict:
    """Per-channel statistics of an image feature from raw uint8 frames [H, W, 3] (a sample),
    pixels scaled to [0, 1], shaped (3, 1, 1) as LeRobot keeps them; also the raw sums so episode
    statistics can be merged into the dataset's."""
    x = np.stack(frames_u8).reshape(-1, 3).astype(np.float64) / 255.0
    shape = lambda v: [[[float(a)]] for a in v]  # noqa: E731
    return {"min": shape(x.min(0)), "max": shape(x.max(0)), "mean": shape(x.mean(0)), "std": shape(x.std(0)),
            "_sum": x.sum(0).tolist(), "_sumsq": (x * x).sum(0).tolist(), "_n": int(len(x))}


def _merge_image_stats(fs: np.ndarray, npx: int) -> dict:
    """Episode image statistics from its frames' [T, 4, 3] statistics (same layout as
    _raw_image_stats, over every pixel of every frame)."""
    mn, mx, sm, sq = fs[:, 0].min(0), fs[:, 1].max(0), fs[:, 2].sum(0), fs[:, 3].sum(0)
    n = npx * len(fs)
    mean = sm / n
    std = np.sqrt(np.maximum(sq / n - mean * mean, 0.0))
    v = np.stack([mn, mx, mean, std]).tolist()  # one conversion, then the (3, 1, 1) nesting
    return {"min": [[[a]] for a in v[0]], "max": [[[a]] for a in v[1]], "mean": [[[a]] for a in v[2]],
            "std": [[[a]] for a in v[3]], "_sum": sm.tolist(), "_sumsq": sq.tolist(), "_n": int(n)}


# ----------------------------------------------------------------------------- LeRobot v3.0 writer
class LeRobotWriter:
    """Streaming LeRobot v3.0 writer (use_videos=False: image features embedded as parquet structs
    {bytes: PNG, path}).  Episodes are added one at a time in episode-index order and appended to
    the open data file (pyarrow ParquetWriter), which rolls over at `data_files_size_in_mb`;
    statistics accumulate as running sums, so memory does not grow with the dataset.

    data/chunk-XXX/file-YYY.parquet  frames of consecutive episodes (features + timestamp,
                                     frame_index, episode_index, index, task_index)
    meta/info.json, meta/tasks.parquet, meta/episodes/chunk-000/file-000.parquet, meta/stats.json
    """

    def __init__(self, root: str, repo_id: str, features: dict, *, fps=CONTROL_FPS, robot_type="franka_panda",
                 chunks_size=1000, data_files_size_in_mb=100, threaded=False, queue_depth=64,
                 image_compression="SNAPPY", keep_image_sums=False, io_threads=None, batch_episodes=64,
                 batch_mb=64):
        import pyarrow as pa
        import pyarrow.compute  # noqa: F401  (imported here, not on the first episode)
        import pyarrow.parquet  # noqa: F401

        self.pa = pa
        self.root, self.repo_id, self.features, self.fps = root, repo_id, features, fps
        self.robot_type, self.chunks_size, self.data_files_size_in_mb = robot_type, chunks_size, data_files_size_in_mb
        os.makedirs(root, exist_ok=True)
        self.num_keys = [k for k, f in features.items() if f["dtype"] == "float32"]
        self.str_keys = [k for k, f in features.items() if f["dtype"] == "string"]
        self.img_keys = [k for k, f in features.items() if f["dtype"] == "image"]
        self.img_type = pa.struct([("bytes", pa.binary()), ("path", pa.string())])
        self.tasks, self.task_idx = [], {}
        self.ep_rows = []
        self.chunk, self.fileno, self.start = 0, 0, 0
        self.writer, self.cur_bytes = None, 0  # the open data file (its path) and its bytes so far
        self.limit = data_files_size_in_mb * 1024 * 1024
        # numeric features' running [min, max, sum, sumsq, count] over the concatenation of their
        # dims (num_keys order, _num_dims each): one set of vector ops per episode, split per feature
        # at close (elementwise, so bit-identical to per-feature accumulators)
        self._num_dims = [int(np.prod(features[k]["shape"])) for k in self.num_keys]
        self.num_acc = None
        self.img_acc = {}  # feature -> [min, max, sum, sumsq, pixels, frames]
        self.n_episodes = 0
        # seconds spent per part of the writer (diagnostics, tools/dataset_bench.py): episode
        # statistics + rows, arrow table building, waiting for a free I/O slot, parquet encode + write
        import threading as _threading

        self.timing = {"episode_stats_s": 0.0, "table_build_s": 0.0, "io_slot_wait_s": 0.0, "io_write_s": 0.0}
        self._timing_lock = _threading.Lock()
        # episodes are encoded in batches (one arrow table / parquet row group per run of episodes
        # that land in the same data file): the per-table arrow overhead is paid once per batch
        self.batch_episodes, self.batch_bytes = max(1, int(batch_episodes)), float(batch_mb) * 1024 * 1024
        self.pending, self.pending_bytes = [], 0
        self._frame_names = []  # "/frame_000000.png", ... (the image paths' per-frame suffixes)
        self.image_compression = image_compression
        # shards keep each episode's raw image sums in meta/episodes, so merge_shards rebuilds the
        # dataset statistics bit for bit
        self.keep_image_sums = keep_image_sums
        # threaded: episodes go through a bounded queue to one writer thread (the reference writes
        # with background threads too, generate_dataset.py:260); parquet encoding and the file write
        # release the GIL, so they overlap the collection loop.  Episode order is kept.
        # parquet encoding + file writes of consecutive data files run on `io_threads` single-thread
        # lanes (file f on lane f mod io_threads, so one file's row groups stay in episode order and
        # files are written side by side; the encoding releases the GIL); episodes, statistics and
        # meta rows stay in order on the collecting thread.  At most 64 tables are in flight.
        self.io_threads = (4 if threaded else 1) if io_threads is None else max(1, int(io_threads))
        self._lanes, self._files, self._futs, self._nfile = None, {}, [], 0
        if self.io_threads > 1:
            import threading
            from concurrent.futures import ThreadPoolExecutor

            self._lanes = [ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"lerobot-io{k}")
                           for k in range(self.io_threads)]
            self._inflight = threading.BoundedSemaphore(64)
        self._q, self._thread, self._err = None, None, None
        if threaded:
            import queue
            import threading

            self._q = queue.Queue(maxsize=queue_depth)
            self._thread = threading.Thread(target=self._drain, name="lerobot-writer", daemon=True)
            self._thread.start()

    def _drain(self):
        while True:
            ep = self._q.get()
            if ep is None:
                return
            if self._err is None:
                try:
                    self._add(ep)
                except BaseException as ex:  # re-raised on the caller's thread
                    self._err = ex

    def _raise_pending(self):
        if self._err is not None:
            err, self._err = self._err, None
            raise err

    def _task(self, ep):
        t = make_task_string(ep.obj, ep.bin)
        if t not in self.task_idx:
            self.task_idx[t] = len(self.tasks)
            self.tasks.append(t)
        return t

    def _table(self, eps, starts):
        """One arrow table holding the frames of consecutive episodes `eps` (dataset indices from
        `starts`)."""
        pa = self.pa
        lens = [ep.length for ep in eps]
        cols, fields = {}, []
        for k in self.num_keys:
            dim = int(np.prod(self.features[k]["shape"]))
            arr = np.concatenate([np.asarray(ep.frames[k], np.float32).reshape(ep.length, dim) for ep in eps])
            cols[k] = pa.FixedSizeListArray.from_arrays(pa.array(arr.ravel(), pa.float32()), dim)
            fields.append(pa.field(k, pa.list_(pa.float32(), dim)))
        for k in self.str_keys:
            cols[k] = pa.array([v for ep in eps for v in ep.frames[k]], pa.string())
            fields.append(pa.field(k, pa.string()))
        nmax = max(lens) if lens else 0
        if len(self._frame_names) < nmax:
            self._frame_names = [f"/frame_{i:06d}.png" for i in range(max(nmax, 2 * len(self._frame_names)))]
        fn = self._frame_names
        fi = np.concatenate([np.arange(L, dtype=np.int64) for L in lens])
        ei = np.repeat(np.arange(len(eps), dtype=np.int64), lens)
        names = pa.array(fn[:nmax], pa.string()).take(pa.array(fi))  # "/frame_000000.png", ... per frame
        for k in self.img_keys:  # LeRobot's embedded image layout (images/<key>/episode_<e>/frame_<i>.png)
            pre = pa.array([f"images/{k}/episode_{ep.index:06d}" for ep in eps], pa.string()).take(pa.array(ei))
            paths = pa.compute.binary_join_element_wise(pre, names, "")  # joined in arrow, not per frame in Python
            if all(isinstance(ep.frames[k], PngFrames) for ep in eps):
                # one chunk per episode straight over its PngFrames buffer (zero-copy)
                chunks, o = [], 0
                for ep in eps:
                    fr = ep.frames[k]
                    if fr.nbytes >= 1 << 31:
                        raise ValueError("an episode's PNG files exceed arrow's 32-bit binary offsets")
                    b = pa.Array.from_buffers(pa.binary(), len(fr), [None, pa.py_buffer(fr.offsets.astype(np.int32)),
                                                                     pa.py_buffer(fr.data)])
                    chunks.append(pa.StructArray.from_arrays([b, paths.slice(o, len(fr))], fields=list(self.img_type)))
                    o += len(fr)
                cols[k] = pa.chunked_array(chunks, type=self.img_type)
            else:
                cols[k] = pa.StructArray.from_arrays([pa.array([v for ep in eps for v in ep.frames[k]], pa.binary()),
                                                      paths], fields=list(self.img_type))
            fields.append(pa.field(k, self.img_type))
        extra = {"timestamp": pa.array((fi / self.fps).astype(np.float32)), "frame_index": pa.array(fi),
                 "episode_index": pa.array(np.repeat(np.array([ep.index for ep in eps], np.int64), lens)),
                 "index": pa.array(np.concatenate([st + np.arange(L, dtype=np.int64) for st, L in zip(starts, lens)])),
                 "task_index": pa.array(np.repeat(np.array([self.task_idx[make_task_string(ep.obj, ep.bin)] for ep in eps],
                                                           np.int64), lens))}
        for k, v in extra.items():
            cols[k] = v
            fields.append(pa.field(k, v.type))
        return pa.Table.from_arrays([cols[f.name] for f in fields], schema=pa.schema(fields))

    def _episode_bytes(self, ep):
        """An episode's size in the data file (the roll-over test): its column data."""
        n = 4 * ep.length * sum(self._num_dims)
        for k in self.str_keys:
            n += sum(map(len, ep.frames[k])) + 4 * ep.length
        for k in self.img_keys:
            n += _png_nbytes(ep.frames[k]) + 54 * ep.length
        return n + 36 * ep.length

    @staticmethod
    def _leaf_columns(schema):
        """Parquet leaf column paths ("a.list.element", "img.bytes", ...) of an arrow schema: read
        back from an empty file written with it."""
        import io

        import pyarrow.parquet as pq

        buf = io.BytesIO()
        pq.write_table(schema.empty_table(), buf)
        buf.seek(0)
        ps = pq.ParquetFile(buf).schema
        return [ps.column(i).path for i in range(len(ps))]

    def _io(self, fn, st):
        """Run fn(st) on the open file's I/O lane (st: that file's state), or inline without lanes."""
        if self._lanes is None:
            fn(st)
            return
        t0 = time.perf_counter()
        self._inflight.acquire()
        self.timing["io_slot_wait_s"] += time.perf_counter() - t0
        fut = self._lanes[st["lane"]].submit(fn, st)
        fut.add_done_callback(lambda _f: self._inflight.release())
        self._futs.append(fut)
        if len(self._futs) > 256:  # surface I/O errors early, keep the list short
            for f in [f for f in self._futs if f.done()]:
                f.result()
            self._futs = [f for f in self._futs if not f.done()]

    def _io_wait(self):
        for f in self._futs:
            f.result()
        self._futs = []

    def _close_file(self):
        if self.writer is not None:
            def close(st):
                if st.get("w") is not None:
                    st["w"].close()
                    st["w"] = None

            self._io(close, self.writer)
            self.writer = None
            self.fileno += 1
            if self.fileno >= self.chunks_size:
                self.chunk, self.fileno = self.chunk + 1, 0
            self.cur_bytes = 0

    def add_episode(self, ep):
        """Append one episode (in episode-index order); queued when the writer is threaded."""
        if self._q is not None:
            self._raise_pending()
            self._q.put(ep)
        else:
            self._add(ep)

    def _add(self, ep):
        t0 = time.perf_counter()
        self._task(ep)
        row = {"episode_index": ep.index, "tasks": [make_task_string(ep.obj, ep.bin)], "length": ep.length,
               "data/chunk_index": None, "data/file_index": None, "dataset_from_index": self.start,
               "dataset_to_index": self.start + ep.length, "meta/episodes/chunk_index": 0,
               "meta/episodes/file_index": 0}
        if self.num_keys:  # every numeric feature's statistics from one [length, sum of dims] array
            L = ep.length
            X = np.concatenate([np.asarray(ep.frames[k], np.float64).reshape(L, -1) for k in self.num_keys], axis=1)
            mn, mx, sm = X.min(0), X.max(0), X.sum(0)
            mean = sm / L
            d = X - mean
            std = np.sqrt((d * d).sum(0) / L)  # np.std's two-pass form
            sq = (X * X).sum(0)
            # one list conversion per statistic, then python slices per feature
            lmn, lmx, lmean, lstd = mn.tolist(), mx.tolist(), mean.tolist(), std.tolist()
            o = 0
            for k, n in zip(self.num_keys, self._num_dims):
                row[f"stats/{k}/min"], row[f"stats/{k}/max"] = lmn[o:o + n], lmx[o:o + n]
                row[f"stats/{k}/mean"], row[f"stats/{k}/std"] = lmean[o:o + n], lstd[o:o + n]
                row[f"stats/{k}/count"] = [int(L)]
                o += n
            acc = self.num_acc
            self.num_acc = [mn, mx, sm, sq, L] if acc is None else \
                [np.minimum(acc[0], mn), np.maximum(acc[1], mx), acc[2] + sm, acc[3] + sq, acc[4] + L]
        for k in self.img_keys:
            st = (getattr(ep, "image_stats", None) or {}).get(k)
            if st is None:  # episodes built elsewhere: decode a frame sample
                st = _raw_image_stats([png_decode(ep.frames[k][i])
                                       for i in np.linspace(0, ep.length - 1, min(ep.length, 8)).astype(int)])
            for name in ("min", "max", "mean", "std"):
                row[f"stats/{k}/{name}"] = st[name]
            row[f"stats/{k}/count"] = [int(ep.length)]
            if self.keep_image_sums:
                row[f"stats/{k}/_sum"], row[f"stats/{k}/_sumsq"] = list(st["_sum"]), list(st["_sumsq"])
                row[f"stats/{k}/_n"] = int(st["_n"])
            mn = np.array([c[0][0] for c in st["min"]])
            mx = np.array([c[0][0] for c in st["max"]])
            acc = self.img_acc.get(k)
            vals = [mn, mx, np.array(st["_sum"]), np.array(st["_sumsq"]), st["_n"], ep.length]
            self.img_acc[k] = vals if acc is None else [np.minimum(acc[0], mn), np.maximum(acc[1], mx), acc[2] + vals[2],
                                                        acc[3] + vals[3], acc[4] + vals[4], acc[5] + vals[5]]
        self.ep_rows.append(row)
        nb = self._episode_bytes(ep)
        self.timing["episode_stats_s"] += time.perf_counter() - t0
        self.pending.append((ep, row, self.start, nb))
        self.pending_bytes += nb
        self.start += ep.length
        self.n_episodes += 1
        if len(self.pending) >= self.batch_episodes or self.pending_bytes >= self.batch_bytes:
            self._flush()

    def _flush(self):
        """Write the pending episodes: each goes to the open data file unless its bytes would take
        the file past data_files_size_in_mb (then the file is closed and the next one opened); the
        episodes of one file are written as one table."""
        import pyarrow.parquet as pq

        pending, self.pending, self.pending_bytes = self.pending, [], 0
        run = []

        def emit():
            if not run:
                return
            t0 = time.perf_counter()
            tab = self._table([r[0] for r in run], [r[2] for r in run])
            self.timing["table_build_s"] += time.perf_counter() - t0
            if self.writer is None:
                d = os.path.join(self.root, "data", f"chunk-{self.chunk:03d}")
                os.makedirs(d, exist_ok=True)
                # PNG bytes are unique per frame: no dictionary attempt on them; their compression is
                # `image_compression` (SNAPPY, parquet's and LeRobot's default, still saves ~17 % on the
                # fixed-Huffman PNGs; NONE writes faster), the other columns keep dictionary + snappy
                plain = [c for c in tab.column_names if c not in self.img_keys]
                comp = {c: (self.image_compression if c.endswith(".bytes") and c[:-6] in self.img_keys else "SNAPPY")
                        for c in self._leaf_columns(tab.schema)}
                path = os.path.join(d, f"file-{self.fileno:03d}.parquet")
                self.writer = {"path": path, "lane": self._nfile % self.io_threads, "w": None,
                               "schema": tab.schema, "kw": dict(use_dictionary=plain, compression=comp)}
                self._nfile += 1

            def write(st, tab=tab):
                t1 = time.perf_counter()
                if st["w"] is None:
                    st["w"] = pq.ParquetWriter(st["path"], st["schema"], **st["kw"])
                st["w"].write_table(tab)
                with self._timing_lock:
                    self.timing["io_write_s"] += time.perf_counter() - t1

            self._io(write, self.writer)
            run.clear()

        for item in pending:
            ep, row, start, nb = item
            if self.cur_bytes > 0 and self.cur_bytes + nb > self.limit:
                emit()
                self._close_file()
            row["data/chunk_index"], row["data/file_index"] = self.chunk, self.fileno
            run.append(item)
            self.cur_bytes += nb
        emit()

    def close(self, extra_info=None):
        import pyarrow as pa
        import pyarrow.parquet as pq

        if self._q is not None:
            self._q.put(None)
            self._thread.join()
            self._q, self._thread = None, None
            self._raise_pending()
        self._flush()
        self._close_file()
        if self._lanes is not None:
            self._io_wait()
            for lane in self._lanes:
                lane.shutdown(wait=True)
            self._lanes = None
        meta = os.path.join(self.root, "meta")
        os.makedirs(os.path.join(meta, "episodes", "chunk-000"), exist_ok=True)
        rows = sorted(self.ep_rows, key=lambda r: r["episode_index"])
        pq.write_table(pa.Table.from_pylist(rows), os.path.join(meta, "episodes", "chunk-000", "file-000.parquet"))
        pq.write_table(pa.table({"task_index": pa.array(np.arange(len(self.tasks), dtype=np.int64)),
                                 "task": pa.array(self.tasks, pa.string())}), os.path.join(meta, "tasks.parquet"))
        stats = {}
        o = 0
        for k, nd in zip(self.num_keys, self._num_dims) if self.num_acc is not None else ():
            mn, mx, sm, sq, n = [a[o:o + nd] for a in self.num_acc[:4]] + [self.num_acc[4]]
            o += nd
            mean = sm / n
            stats[k] = {"min": mn.tolist(), "max": mx.tolist(), "mean": mean.tolist(),
                        "std": np.sqrt(np.maximum(sq / n - mean * mean, 0.0)).tolist(), "count": [int(n)]}
        shape = lambda v: [[[float(a)]] for a in v]  # noqa: E731
        for k, (mn, mx, sm, sq, npx, nfr) in self.img_acc.items():
            mean = sm / npx
            stats[k] = {"min": shape(mn), "max": shape(mx), "mean": shape(mean),
                        "std": shape(np.sqrt(np.maximum(sq / npx - mean * mean, 0.0))), "count": [int(nfr)]}
        with open(os.path.join(meta, "stats.json"), "w") as f:
            json.dump(stats, f, indent=1)
        feats = {k: {"dtype": v["dtype"], "shape": list(v["shape"]), "names": v["names"]}
                 for k, v in self.features.items()}
        for k, dt in (("timestamp", "float32"), ("frame_index", "int64"), ("episode_index", "int64"),
                      ("index", "int64"), ("task_index", "int64")):
            feats[k] = {"dtype": dt, "shape": [1], "names": None}
        info = {"codebase_version": "v3.0", "robot_type": self.robot_type, "total_episodes": self.n_episodes,
                "total_frames": int(self.start), "total_tasks": len(self.tasks), "chunks_size": self.chunks_size,
                "data_files_size_in_mb": self.data_files_size_in_mb, "video_files_size_in_mb": 500, "fps": self.fps,
                "splits": {"train": f"0:{self.n_episodes}"},
                "data_path": "data/chunk-{chunk_index:03d}/file-{file_index:03d}.parquet", "video_path": None,
                "features": feats}
        if extra_info:
            info.update(extra_info)
        with open(os.path.join(meta, "info.json"), "w") as f:
            json.dump(info, f, indent=4)
        return info


def write_lerobot_v3(root: str, repo_id: str, episodes, features: dict, *, fps=CONTROL_FPS,
                     robot_type="franka_panda", chunks_size=1000, data_files_size_in_mb=100, extra_info=None):
    """Write a list of episodes in the LeRobot v3.0 layout (LeRobotWriter, episodes in index order)."""
    w = LeRobotWriter(root, repo_id, features, fps=fps, robot_type=robot_type, chunks_size=chunks_size,
                      data_files_size_in_mb=data_files_size_in_mb)
    for ep in sorted(episodes, key=lambda e: e.index):
        w.add_episode(ep)
    return w.close(extra_info)


def read_lerobot_v3(root: str):
    """Load the frames written by write_lerobot_v3 -> (info, metadata or None, {episode: {feature: array}})."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    info = json.load(open(os.path.join(root, "meta", "info.json")))
    md_path = os.path.join(root, "metadata.json")
    metadata = json.load(open(md_path)) if os.path.exists(md_path) else None
    eps_tab = pq.read_table(os.path.join(root, "meta", "episodes", "chunk-000", "file-000.parquet")).to_pylist()
    out = {}
    files = {}
    for row in eps_tab:
        key = (row["data/chunk_index"], row["data/file_index"])
        if key not in files:
            p = info["data_path"].format(chunk_index=key[0], file_index=key[1])
            files[key] = pq.read_table(os.path.join(root, p))
        tab = files[key]
        epi = tab.column("episode_index").to_numpy()
        sel = np.where(epi == row["episode_index"])[0]
        fr = {}
        for name in tab.column_names:
            col = tab.column(name).take(sel).combine_chunks()
            if pa.types.is_fixed_size_list(col.type):
                fr[name] = np.asarray(col.flatten(), np.float32).reshape(len(sel), col.type.list_size)
            elif pa.types.is_struct(col.type):  # embedded image: {bytes: PNG, path}
                fr[name] = np.stack([png_decode(v["bytes"]) for v in col.to_pylist()]) if len(sel) else None
            elif pa.types.is_string(col.type):
                fr[name] = col.to_pylist()
            else:
                fr[name] = col.to_numpy()
        out[row["episode_index"]] = fr
    return info, metadata, out


def _shard_episodes(sdir: str, feats: dict, global_ids: list, seeds):
    """Episodes of one shard in its (global-index increasing) order, read file by file: Episode
    objects with their global index, PNG bytes as stored and the image statistics the writer kept."""
    import pyarrow.parquet as pq

    info = json.load(open(os.path.join(sdir, "meta", "info.json")))
    rows = pq.read_table(os.path.join(sdir, "meta", "episodes", "chunk-000", "file-000.parquet")).to_pylist()
    by_task = {make_task_string(o, b): (o, b) for o in OBJECTS for b in BINS}
    cur_key, tab, epi = None, None, None
    for row in sorted(rows, key=lambda r: r["episode_index"]):
        key = (row["data/chunk_index"], row["data/file_index"])
        if key != cur_key:
            cur_key = key
            tab = pq.read_table(os.path.join(sdir, info["data_path"].format(chunk_index=key[0], file_index=key[1])))
            epi = tab.column("episode_index").to_numpy()
        sel = np.where(epi == row["episode_index"])[0]
        g = int(global_ids[row["episode_index"]])
        obj, bin_ = by_task[row["tasks"][0]]
        ep = Episode(g, obj, bin_, int(seeds[g]) if seeds else None, length=int(row["length"]))
        part = tab.take(sel)
        for k, f in feats.items():
            col = part.column(k).combine_chunks()
            if f["dtype"] == "float32":
                ep.frames[k] = np.asarray(col.flatten(), np.float32).reshape(len(sel), -1)
            elif f["dtype"] == "string":
                ep.frames[k] = col.to_pylist()
            else:
                ep.frames[k] = col.field("bytes").to_pylist()
                ep.image_stats[k] = {n: row[f"stats/{k}/{n}"] for n in ("min", "max", "mean", "std", "_sum", "_sumsq",
                                                                        "_n")}
        yield ep


def merge_shards(path: str, remove_shards: bool = False):
    """Merge the LeRobot shards a sharded generate() wrote under `path` into the dataset one
    process would have written there (episodes in global order, global indices, the same
    statistics and metadata bit for bit).  Streams: one data file per shard is held at a time."""
    import heapq
    import shutil

    sdirs = sorted(d for d in (os.path.join(path, x) for x in os.listdir(path)) if os.path.basename(d).startswith("shard-"))
    if not sdirs:
        raise ValueError(f"no shards under {path}")
    mds = [json.load(open(os.path.join(d, "metadata.json"))) for d in sdirs]
    world = mds[0]["shard"]["world_size"]
    if len(sdirs) != world or sorted(m["shard"]["rank"] for m in mds) != list(range(world)):
        raise ValueError(f"expected {world} shards, found ranks {[m['shard']['rank'] for m in mds]}")
    cfg = {k: v for k, v in mds[0].items() if k != "shard"}
    feats = _features_at(resolve_features(cfg["features"], cfg["reward_type"]), cfg.get("image_size", IMAGE_SIZE))
    seeds = cfg.get("episode_seeds")
    writer = LeRobotWriter(path, cfg["repo_id"], feats, threaded=True)
    streams = [_shard_episodes(d, feats, m["shard"]["global_episode_index"], seeds) for d, m in zip(sdirs, mds)]
    n = 0
    for ep in heapq.merge(*streams, key=lambda e: e.index):
        if ep.index != n:
            raise ValueError(f"episode {n} missing from the shards (next is {ep.index})")
        writer.add_episode(ep)
        n += 1
    if n != cfg["num_episodes"]:
        raise ValueError(f"shards hold {n} of {cfg['num_episodes']} episodes")
    info = writer.close(extra_info={"generation_config": cfg})
    with open(os.path.join(path, "metadata.json"), "w") as f:
        json.dump(cfg, f, indent=2)
    if remove_shards:
        for d in sdirs:
            shutil.rmtree(d)
    return info
