"""The prefix decode continued (himg_hip_decode_prefix_more_*, himg_hip_prefix_peek_from) as its definition
in include/himg_hip.h, in plain Python on tests/prefix_model.py: the state, the rules a state must pass, the
row walk RESUMED at a state -- written out here, not a call of the walk from scratch --, and one step of a
chain: what a call returns, which block rows it writes, the state it leaves.

Test infrastructure only.
"""
import prefix_model as pm

ARG = -1
FRESH = dict(started=0, rows_done=0, walk_pos=0, avail_seen=0)


def state(started=0, rows_done=0, walk_pos=0, avail_seen=0):
    return dict(started=started, rows_done=rows_done, walk_pos=walk_pos, avail_seen=avail_seen)


def _rows_from(b, fix_t2, p, q, r0, end):
    """prefix_model._rows with the walk standing at q, r0 rows behind it.  Sets rows_complete, used_bytes and
    next_bytes of p; returns the (payload offset, length) of the rows it passed, rows r0 .. k - 1."""
    avail, T, rows = len(b), p["packed_size"], p["rows"]
    p.update(rows_complete=r0, used_bytes=q, next_bytes=T)
    new = []
    if fix_t2 and rows == 1:   # one block row has no size header
        if r0 == 0:
            if end <= avail:
                p.update(rows_complete=1, used_bytes=end)
                new.append((q, end - q))
            else:
                p["next_bytes"] = end
        return new
    r, cut = r0, False
    while q != end:
        if q + 2 > end:
            raise pm._Format
        if q + 2 > avail:
            cut, p["next_bytes"] = True, q + 2
            break
        n, body = b[q] | (b[q + 1] << 8), q + 2
        if n & 0x8000:
            if body + 2 > end:
                raise pm._Format
            if body + 2 > avail:
                cut, p["next_bytes"] = True, body + 2
                break
            n = (n & 0x7fff) | ((b[body] | (b[body + 1] << 8)) << 15)
            body += 2
        if n > end - body:
            raise pm._Format
        if body + n > avail:
            cut, p["next_bytes"] = True, body + n
            break
        if r < rows:
            p["used_bytes"] = body + n
            new.append((body, n))
        r += 1
        q = body + n
    if not cut and r < rows:
        raise pm._Format   # fewer blocks than block rows
    p["rows_complete"] = min(r, rows)
    if p["rows_complete"] == rows:
        p["next_bytes"] = T
    return new


def walk_from(packed, st, avail=None, fix_t2=False):
    """(code, plan) of the first `avail` bytes of `packed`, the row walk resumed at state `st`: what
    himg_hip_prefix_peek_from returns.  A fresh state: prefix_model.walk.  ARG (with an empty plan) for a
    state that cannot be right: avail below avail_seen -- judged before the head --, then, once the head has
    passed, rows_done outside [0, rows], walk_pos outside [head_bytes, the chunk's end], walk_pos > avail."""
    b = bytes(packed[:avail]) if isinstance(packed, bytes) else bytes(packed[:avail].tobytes())
    if not st["started"]:
        return pm.walk(b, len(b), fix_t2)
    if len(b) < st["avail_seen"]:
        return ARG, pm.empty_plan()
    p = pm.empty_plan()
    try:
        q, end = pm._head(b, fix_t2, p)
        if not (0 <= st["rows_done"] <= p["rows"] and q <= st["walk_pos"] <= end and st["walk_pos"] <= len(b)):
            return ARG, pm.empty_plan()
        _rows_from(b, fix_t2, p, st["walk_pos"], st["rows_done"], end)
    except pm._Short:
        return pm.CAPACITY, p
    except pm._Format:
        return pm.FORMAT, p
    return pm.OK, p


def step(model, st, avail):
    """One call at `avail` bytes of model's stream with state `st`: (code, k, rows written, new state).
    rows written: the (first, end) block rows the call stores -- for a fresh state (0, rows), the whole
    picture: rows below k decoded, the others filled --, None where nothing is written.  A call with a
    verdict leaves the state as it was and k = -1.  (The rows' entropy checks pass: the model's stream is one
    the decoder accepts.)"""
    code, p = walk_from(model.packed, st, avail, model.fix_t2)
    if code:
        return code, -1, None, dict(st)
    k = p["rows_complete"]
    new = state(1, k, p["used_bytes"], avail)
    if not st["started"]:
        return pm.OK, k, (0, model.rows), new
    return pm.OK, k, ((st["rows_done"], k) if k > st["rows_done"] else None), new


def mixed_batch(model):
    """Six (state, avail, code) for ONE launch over model's stream (five block rows): the kinds of frame the
    gate must keep apart when they share its per-frame words.  code: what step() must say of each.  The
    resumed states are the model's own, each reached by one step from a fresh one."""
    e = model.row_ends()
    assert len(e) == 6 and model.T // 2 > e[1]
    rows_st = step(model, state(), e[1] + 1)[3]      # one row done, the walk behind it
    idle_st = step(model, state(), e[2] + 3)[3]      # two rows done, three bytes of the next header seen
    return [(state(), model.T // 2, pm.OK),                # fresh, about half the stream
            (rows_st, e[3], pm.OK),                        # resumed: rows 1 and 2 are new
            (idle_st, e[2] + 3, pm.OK),                    # resumed: no new bytes
            (state(), e[0] - 1, pm.CAPACITY),              # the bytes end inside the head
            (state(1, 3, e[3], e[1]), e[2], ARG),          # resumed, walk_pos beyond avail
            (state(), model.T, pm.OK)]                     # fresh, the whole stream
