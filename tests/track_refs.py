"""Float64 references for row f-5 (tracking): SORT exactly as DESIGN.md section 3 freezes it, its optimal assignment, the CLEAR MOT metric
and the seeded scene generator the tests share.  Plain statements, sharing no code with the product:

* `SortRef` carries the FULL 7-state Kalman filter with 7 x 7 matrices (the kernel runs three 2-state filters and a scalar one: the shortcut is
  checked against the general filter, `decoupling_residual`).  `dtype=np.float32` runs the same statements in float32 -- the tests take the
  float32 run's own deviation from the float64 run as the measure of what an fp32 implementation may deviate.
* `assign_max` is an O(n^3) shortest-augmenting-path assignment written here, `assign_brute` the permutation search for n <= 7.
* `kept(seed, direct)`: a generated case is used for decision tests iff no positive IoU the reference sees lies within 1e-4 of the threshold
  and three reruns with every positive IoU perturbed by U(-1e-5, 1e-5) decide identically -- a correct fp32 kernel cannot fail such a case on
  a coin-flip.
"""
import itertools

import numpy as np

IOU_THR = 0.3
MARGIN = 1e-4
PERTURB = 1e-5
N_FRAMES = 24
N_OBJ = 12


# ---- assignment ---------------------------------------------------------------------------------------------------------------------------
def _assign_rows_le_cols(cost):
    """min-cost assignment of every row of cost (n x m, n <= m): potentials + shortest augmenting paths.  -> column of each row."""
    n, m = cost.shape
    INF = float("inf")
    u = np.zeros(n + 1)
    v = np.zeros(m + 1)
    p = np.zeros(m + 1, dtype=np.int64)          # p[j] = row (1-based) in column j; column 0 is virtual
    way = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, INF)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = np.full(m + 1, INF)
            cur[1:] = cost[i0 - 1] - u[i0] - v[1:]
            better = free & (cur < minv)
            minv[better] = cur[better]
            way[better] = j0
            cand = np.where(free, minv, INF)
            j1 = int(np.argmin(cand))
            delta = cand[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = np.full(n, -1, dtype=np.int64)
    for j in range(1, m + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def assign_max(M):
    """The assignment of min(rows, cols) pairs that maximises the summed entries of M.  -> list of (row, col), rows ascending."""
    M = np.asarray(M, dtype=np.float64)
    nr, nc = M.shape
    if nr == 0 or nc == 0:
        return []
    if nr <= nc:
        col = _assign_rows_le_cols(-M)
        return [(r, int(c)) for r, c in enumerate(col)]
    col = _assign_rows_le_cols(-M.T)
    return sorted((int(r), c) for c, r in enumerate(col))


def assign_brute(M):
    """The optimum of assign_max by exhaustive search (min(rows, cols) <= 7).  -> the best total."""
    M = np.asarray(M, dtype=np.float64)
    nr, nc = M.shape
    if nr == 0 or nc == 0:
        return 0.0
    if nr > nc:
        M, nr, nc = M.T, nc, nr
    best = -float("inf")
    for cols in itertools.permutations(range(nc), nr):
        best = max(best, float(sum(M[r, c] for r, c in enumerate(cols))))
    return best


def associate(M, thr=IOU_THR, direct=True):
    """The association rule: row_to_col (int64 [rows], -1 = unmatched).  Non-finite entries read as 0."""
    M = np.array(M, dtype=np.float64)
    M[~np.isfinite(M)] = 0.0
    nr, nc = M.shape
    out = np.full(nr, -1, dtype=np.int64)
    if nr == 0 or nc == 0:
        return out
    if direct:
        a = M > thr
        if a.sum(1).max() <= 1 and a.sum(0).max() <= 1:
            r, c = np.nonzero(a)
            out[r] = c
            return out
    for r, c in assign_max(M):
        if not M[r, c] < thr:
            out[r] = c
    return out


def matching_total(M, row_to_col):
    M = np.asarray(M, dtype=np.float64)
    return float(sum(M[r, c] for r, c in enumerate(row_to_col) if c >= 0))


def is_partial_matching(row_to_col, n_rows, n_cols):
    cols = [int(c) for c in row_to_col[:n_rows] if c >= 0]
    return (all(0 <= c < n_cols for c in cols) and len(set(cols)) == len(cols)
            and all(int(c) == -1 for c in row_to_col[n_rows:]))


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------
def iou_xyxy(a, b, dtype=np.float64):
    """IoU of axis-aligned boxes a [D][4] against b [T][4] -> [D][T] (abewley's iou_batch)."""
    a = np.asarray(a, dtype=dtype).reshape(-1, 4)
    b = np.asarray(b, dtype=dtype).reshape(-1, 4)
    a = a[:, None, :]
    b = b[None, :, :]
    w = np.maximum(dtype(0), np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    h = np.maximum(dtype(0), np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    wh = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        o = wh / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - wh)
    return o


def box_to_z(b, dtype=np.float64):
    b = np.asarray(b, dtype=dtype)
    w = b[2] - b[0]
    h = b[3] - b[1]
    return np.array([b[0] + w / dtype(2), b[1] + h / dtype(2), w * h, w / h], dtype=dtype)


def x_to_box(x):
    dtype = x.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.sqrt(x[2] * x[3])
        h = x[2] / w
    return np.array([x[0] - w / dtype(2), x[1] - h / dtype(2), x[0] + w / dtype(2), x[1] + h / dtype(2)], dtype=x.dtype)


# ---- SORT ---------------------------------------------------------------------------------------------------------------------------------
P_INDEX = ((0, 0), (0, 4), (4, 4), (1, 1), (1, 5), (5, 5), (2, 2), (2, 6), (6, 6), (3, 3))     # the ten entries the C ABI stores, in its order
_PATTERN = np.zeros((7, 7), dtype=bool)
for _i, _j in P_INDEX:
    _PATTERN[_i, _j] = _PATTERN[_j, _i] = True


class _Track:
    __slots__ = ("x", "P", "id", "tsu", "hits", "streak", "age")


class SortRef:
    """One stream.  step(dets_xyxy) -> (boxes [k][4], ids [k], det_index [k]) in ascending id."""

    def __init__(self, max_age=1, min_hits=3, iou_thr=IOU_THR, t_cap=64, direct=True, dtype=np.float64, perturb_rng=None):
        self.max_age, self.min_hits, self.thr, self.t_cap, self.direct, self.dtype = max_age, min_hits, iou_thr, t_cap, bool(direct), dtype
        self.perturb_rng = perturb_rng
        self.tracks = []
        self.next_id = 0           # ids given so far
        self.frame_count = 0
        self.status = 0
        self.seen_iou = []         # every positive IoU an association looked at
        self.readings_differ = 0   # frames on which direct = 0 and direct = 1 decide differently on THIS run's matrix
        self.offpattern = 0.0      # largest |P| entry outside the pattern the kernel stores
        d = dtype
        self.F = np.eye(7, dtype=d)
        self.F[0, 4] = self.F[1, 5] = self.F[2, 6] = 1
        self.H = np.eye(7, dtype=d)[:4]
        self.R = np.diag(np.array([1, 1, 10, 10], dtype=d))
        self.Q = np.diag(np.array([1, 1, 1, 1, 0.01, 0.01, 1e-4], dtype=d))
        self.P0 = np.diag(np.array([10, 10, 10, 10, 1e4, 1e4, 1e4], dtype=d))

    def _note(self, P):
        self.offpattern = max(self.offpattern, float(np.abs(np.where(_PATTERN, 0, P)).max()))

    def step(self, dets, det_count=None):
        d = self.dtype
        dets = np.asarray(dets, dtype=d).reshape(-1, 4)
        n = len(dets) if det_count is None else det_count
        if n < 0:
            self.status |= 4
            n = 0
        if n > min(64, len(dets)):
            self.status |= 1
            n = min(64, len(dets))
        dets = dets[:n]
        self.frame_count += 1
        # predict
        live, pred = [], []
        for t in self.tracks:
            if t.x[6] + t.x[2] <= 0:
                t.x[6] = 0
            t.x = self.F @ t.x
            t.P = self.F @ t.P @ self.F.T + self.Q
            self._note(t.P)
            t.age += 1
            if t.tsu > 0:
                t.streak = 0
            t.tsu += 1
            b = x_to_box(t.x)
            if np.all(np.isfinite(b)):
                live.append(t)
                pred.append(b)
        self.tracks = live
        # associate
        M = iou_xyxy(dets, np.array(pred, dtype=d).reshape(-1, 4), d).astype(np.float64)
        M[~np.isfinite(M)] = 0.0
        if self.perturb_rng is not None:
            M = np.where(M > 0, M + self.perturb_rng.uniform(-PERTURB, PERTURB, M.shape), M)
        self.seen_iou.extend(M[M > 0].tolist())
        r2c = associate(M, self.thr, self.direct)
        if M.size and not np.array_equal(r2c, associate(M, self.thr, not self.direct)):
            self.readings_differ += 1
        # update
        matched_det = {}
        for r, c in enumerate(r2c):
            if c < 0:
                continue
            t = self.tracks[c]
            matched_det[t.id] = r
            t.tsu = 0
            t.hits += 1
            t.streak += 1
            z = box_to_z(dets[r], d)
            y = z - self.H @ t.x
            S = self.H @ t.P @ self.H.T + self.R
            K = t.P @ self.H.T @ np.linalg.inv(S)
            t.x = t.x + K @ y
            A = np.eye(7, dtype=d) - K @ self.H
            t.P = A @ t.P @ A.T + K @ self.R @ K.T
            self._note(t.P)
        # births
        for r, c in enumerate(r2c):
            if c >= 0:
                continue
            if len(self.tracks) >= self.t_cap:
                self.status |= 2
                continue
            t = _Track()
            t.x = np.concatenate([box_to_z(dets[r], d), np.zeros(3, dtype=d)])
            t.P = self.P0.copy()
            self.next_id += 1
            t.id, t.tsu, t.hits, t.streak, t.age = self.next_id, 0, 0, 0, 0
            matched_det[t.id] = r
            self.tracks.append(t)
        # output, deaths
        out = [(x_to_box(t.x), t.id, matched_det[t.id]) for t in self.tracks
               if t.tsu == 0 and (t.streak >= self.min_hits or self.frame_count <= self.min_hits)]
        self.tracks = [t for t in self.tracks if t.tsu <= self.max_age]
        boxes = np.array([o[0] for o in out], dtype=d).reshape(-1, 4)
        return boxes, np.array([o[1] for o in out], dtype=np.int64), np.array([o[2] for o in out], dtype=np.int64)

    # the C ABI's view of the state
    def stream_i(self):
        return np.array([len(self.tracks), self.next_id, self.frame_count, self.status], dtype=np.int64)

    def trk_i(self):
        return np.array([[t.id, t.tsu, t.hits, t.streak, t.age] for t in self.tracks], dtype=np.int64).reshape(-1, 5)

    def trk_f(self):
        return np.array([list(t.x) + [t.P[i, j] for i, j in P_INDEX] for t in self.tracks], dtype=np.float64).reshape(-1, 17)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def make_case(seed, n_obj=N_OBJ, n_frames=N_FRAMES):
    """-> (dets: list of float32 [k][4] per frame, gt: float64 [frames][n_obj][4]).  Detections are float32 so that every implementation
    starts from the same numbers; ground truth = the noise-free boxes of ALL objects, id = object index."""
    rng = np.random.default_rng(1000 + seed)
    pos = rng.uniform(-28, 28, (n_obj, 2))
    vel = rng.uniform(-1.5, 1.5, (n_obj, 2))
    size = np.stack([rng.uniform(3.5, 5.5, n_obj), rng.uniform(1.7, 2.4, n_obj)], 1)
    if seed % 2:
        size = size[:, ::-1]
    dets, gt = [], np.zeros((n_frames, n_obj, 4))
    for f in range(n_frames):
        c = pos + vel * f
        gt[f] = np.concatenate([c - size / 2, c + size / 2], 1)
        rows = []
        for o in range(n_obj):
            drop = rng.random() < 0.12
            cn = c[o] + rng.normal(0, 0.08, 2)
            sz = size[o] * (1 + 0.02 * rng.normal(0, 1, 2))
            if not drop:
                rows.append(np.concatenate([cn - sz / 2, cn + sz / 2]))
        for _ in range(int(rng.integers(0, 3))):
            cn = rng.uniform(-28, 28, 2)
            sz = rng.uniform(1.5, 5, 2)
            rows.append(np.concatenate([cn - sz / 2, cn + sz / 2]))
        rows = np.array(rows, dtype=np.float64).reshape(-1, 4)
        rows = rows[rng.permutation(len(rows))]
        dets.append(rows.astype(np.float32))
    return dets, gt


def run_case(dets, direct=True, dtype=np.float64, perturb_rng=None, **kw):
    """The whole sequence through one SortRef.  -> (tracker, per-frame records); a record holds everything the tests compare."""
    trk = SortRef(direct=direct, dtype=dtype, perturb_rng=perturb_rng, **kw)
    frames = []
    for d in dets:
        boxes, ids, det = trk.step(d)
        frames.append({"boxes": boxes.astype(np.float64), "ids": ids, "det": det, "stream_i": trk.stream_i(), "trk_i": trk.trk_i(), "trk_f": trk.trk_f()})
    return trk, frames


def decisions(frames):
    """The integer content of a run (what must be EQUAL between two correct implementations)."""
    return [(f["ids"].tolist(), f["det"].tolist(), f["stream_i"].tolist(), f["trk_i"].tolist()) for f in frames]


_KEPT = {}


def kept(seed, direct):
    """See the module docstring.  Cached: the GPU tests and the CPU tests share the answer."""
    key = (seed, bool(direct))
    if key not in _KEPT:
        dets, _ = make_case(seed)
        trk, frames = run_case(dets, direct)
        ok = not any(abs(v - IOU_THR) < MARGIN for v in trk.seen_iou)
        base = decisions(frames)
        for k in range(3):
            if not ok:
                break
            _, fr = run_case(dets, direct, perturb_rng=np.random.default_rng(7000 + 10 * seed + k))
            ok = decisions(fr) == base
        _KEPT[key] = ok
    return _KEPT[key]


def kept_seeds(direct, count, upto=40):
    out = [s for s in range(upto) if kept(s, direct)]
    return out[:count]


# ---- CLEAR MOT (TrackEval's clear.py) -----------------------------------------------------------------------------------------------------
class ClearMotRef:
    def __init__(self, thr=0.5):
        self.thr = thr
        self.tp = self.fn = self.fp = self.idsw = 0
        self.iou_sum = 0.0
        self.prev = {}              # gt id -> the tracker id of its last match, any frame back
        self.prev_step = {}         # gt id -> the tracker id of its match in the previous frame

    def update(self, gt_boxes, gt_ids, trk_boxes, trk_ids):
        gt_ids = [int(g) for g in gt_ids]
        trk_ids = [int(t) for t in trk_ids]
        ng, nt = len(gt_ids), len(trk_ids)
        if ng == 0 or nt == 0:
            self.fn += ng
            self.fp += nt
            self.prev_step = {}
            return
        sim = iou_xyxy(gt_boxes, trk_boxes)
        sim[~np.isfinite(sim)] = 0.0
        eps = np.finfo(np.float64).eps
        score = np.array([[1000.0 * (self.prev_step.get(g) == t) for t in trk_ids] for g in gt_ids]) + sim
        score[sim < self.thr - eps] = 0
        step = {}
        for r, c in assign_max(score):
            if score[r, c] > eps:
                g, t = gt_ids[r], trk_ids[c]
                if g in self.prev and self.prev[g] != t:
                    self.idsw += 1
                step[g] = t
                self.iou_sum += float(sim[r, c])
        self.prev.update(step)
        self.prev_step = step
        self.tp += len(step)
        self.fn += ng - len(step)
        self.fp += nt - len(step)

    def result(self):
        gt = self.tp + self.fn
        return {"MOTA": (self.tp - self.fp - self.idsw) / gt if gt else 0.0, "MOTP": self.iou_sum / self.tp if self.tp else 0.0,
                "IDSW": self.idsw, "TP": self.tp, "FP": self.fp, "FN": self.fn}
