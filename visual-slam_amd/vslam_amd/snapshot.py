"""The snapshot of a device map (mo_map_export / mo_map_import in include/vslam_amd.h) as numpy arrays, and the one-file format
LocalMapper.save_state / load_state keep it in.

The file is one .npz read with allow_pickle=False: a format version, the snapshot (`dims` and the arrays under map_*), the camera matrix
and the host's bookkeeping as plain arrays.  check_file checks all of it - version, presence, dtype, shape, mutual consistency - and
needs neither the library nor a GPU; a bad file raises ValueError naming the array."""
import ctypes as C

import numpy as np

import vslam_amd as V

FORMAT_VERSION = 1

# the dims block as an int64 vector, in this order (mo_map_snapshot_dims_t)
DIM_NAMES = ("n_kf", "list_rows", "kf_rows", "n_pts", "n_obs", "list_ids", "kf_stored", "id_bound", "img_w0", "img_w1", "img_h0", "img_h1",
             "img_ch0", "img_ch1", "img_cur", "st_live0", "st_live1", "st_live2", "img_bytes0", "img_bytes1")


def _dims_to_vector(d):
    return np.array([d.n_kf, d.list_rows, d.kf_rows, d.n_pts, d.n_obs, d.list_ids, d.kf_stored, d.id_bound, d.img_w[0], d.img_w[1], d.img_h[0],
                     d.img_h[1], d.img_ch[0], d.img_ch[1], d.img_cur, d.st_live[0], d.st_live[1], d.st_live[2], d.img_bytes[0], d.img_bytes[1]],
                    np.int64)


def _vector_to_dims(v, d):
    g = dict(zip(DIM_NAMES, (int(x) for x in v)))
    for k in ("n_kf", "list_rows", "kf_rows", "n_pts", "n_obs", "list_ids", "kf_stored", "id_bound", "img_cur"):
        setattr(d, k, g[k])
    for i in range(2):
        d.img_w[i], d.img_h[i], d.img_ch[i], d.img_bytes[i] = g["img_w%d" % i], g["img_h%d" % i], g["img_ch%d" % i], g["img_bytes%d" % i]
    for i in range(3):
        d.st_live[i] = g["st_live%d" % i]


def array_specs(dims):
    """{snapshot array: (dtype, shape)} for a dims vector: what mo_map_export fills and mo_map_import reads"""
    g = dict(zip(DIM_NAMES, (int(x) for x in dims)))
    n_kf, rows, n, no, lr = g["n_kf"], g["kf_rows"], g["n_pts"], g["n_obs"], g["list_rows"]
    i4 = np.dtype(np.int32)
    return {"kf_cnt": (i4, (n_kf,)), "kf_ord": (i4, (n_kf,)), "kf_kps": (V.KP_DTYPE, (rows,)), "kf_desc": (np.dtype(np.uint8), (rows, 32)),
            "kf_P": (np.dtype(np.float64), (n_kf, 12)), "xyz": (np.dtype(np.float32), (n, 3)), "col": (np.dtype(np.uint8), (n, 3)), "id": (i4, (n,)),
            "dref_kf": (i4, (n,)), "dref_row": (i4, (n,)), "obs_off": (i4, (n + 1,)), "obs_kf": (i4, (no,)), "obs_kp": (i4, (no,)),
            "life": (i4, (n, 4)), "list_off": (i4, (lr + 1 if lr else 0,)), "list_ids": (i4, (g["list_ids"],)), "kf_red": (i4, (lr,)),
            "img0": (np.dtype(np.uint8), (g["img_bytes0"],)), "img1": (np.dtype(np.uint8), (g["img_bytes1"],))}


def _struct_of(arrays):
    """mo_map_snapshot over the arrays (which must stay alive while it is used)"""
    s = V.MapSnapshot()
    _vector_to_dims(arrays["dims"], s.dims)
    for name in ("kf_cnt", "kf_ord", "kf_kps", "kf_desc", "kf_P", "xyz", "col", "id", "dref_kf", "dref_row", "obs_off", "obs_kf", "obs_kp", "life",
                 "list_off", "list_ids", "kf_red"):
        a = arrays[name]
        setattr(s, name, a.ctypes.data if a.size else None)
    for i in range(2):
        a = arrays["img%d" % i]
        s.img[i] = a.ctypes.data if a.size else None
    return s


def export_map(lib, map_handle, check):
    """{"dims": int64 vector, every snapshot array}: mo_map_snapshot_dims, the arrays allocated, mo_map_export.  check(rc) raises."""
    d = V.MapSnapshotDims()
    check(lib.mo_map_snapshot_dims(map_handle, C.byref(d)))
    arrays = {"dims": _dims_to_vector(d)}
    for name, (dtype, shape) in array_specs(arrays["dims"]).items():
        arrays[name] = np.zeros(shape, dtype)
    s = _struct_of(arrays)
    check(lib.mo_map_export(map_handle, C.byref(s)))
    after = _dims_to_vector(s.dims)
    if not np.array_equal(after, arrays["dims"]):
        raise RuntimeError("the map changed between mo_map_snapshot_dims and mo_map_export")
    return arrays


def import_map(lib, ctx_handle, arrays, capacity, check):
    """a new mo_map from snapshot arrays (mo_map_import); capacity as LocalMapper's: (kf_slots, rows, points, observations)"""
    keep = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
    s = _struct_of(keep)
    h = C.c_void_p()
    kf_slots, rows, pts, obs = capacity
    check(lib.mo_map_import(ctx_handle, C.byref(s), int(kf_slots), int(rows), int(pts), int(obs), C.byref(h)))
    return h


# ---- the file --------------------------------------------------------------------------------------------------------------------------
_I8, _U1, _F8 = np.dtype(np.int64), np.dtype(np.uint8), np.dtype(np.float64)


def host_specs(z):
    """{host array: (dtype, shape)}; None in a shape: any length, further tied to other arrays by check_file"""
    n_kf = int(z["dims"][0])
    return {"camera_matrix": (_F8, (3, 3)), "settings": (_F8, (4,)), "sampling": (np.dtype(np.uint64), (3,)),
            "kf_ids": (_I8, (n_kf,)), "kf_poses": (_F8, (n_kf, 4, 4)), "kf_serials": (_I8, (n_kf,)), "next_serial": (_I8, ()),
            "list_rows": (_I8, (n_kf,)), "covis": (_I8, (None, 3)), "rec_n": (_I8, (None,)),
            "dead_ref": (_I8, (None, 2)), "dead_desc": (_U1, (None, 32)),
            "n_injected": (_I8, ()), "inj_index": (_I8, (None,)), "inj_id": (_I8, (None,)), "inj_pos": (_F8, (None, 3)),
            "inj_flags": (_U1, (None, 3)), "inj_color": (_U1, (None, 3)), "inj_desc": (_U1, (None, 32)), "inj_obs_off": (_I8, (None,)),
            "inj_obs": (_I8, (None, 2)),
            "lc_threshold": (_I8, ()), "lc_counts": (_I8, (None,)), "lc_off": (_I8, (None,)), "lc_serials": (_I8, (None,)),
            "vocab_words": (_U1, (None, 32)), "vocab_weights": (np.dtype(np.int32), (None,)),
            "images_all": (_I8, ()), "image_shapes": (_I8, (None, 3)), "last_image_size": (_I8, (2,))}


def _get(z, name, dtype, shape):
    if name not in z.files:
        raise ValueError("state file: array %r is missing" % name)
    try:
        a = z[name]
    except ValueError as e:   # (an object array: numpy refuses to unpickle it)
        raise ValueError("state file: array %r cannot be read without pickle (%s)" % (name, e)) from None
    if a.dtype == object or a.dtype != dtype:
        raise ValueError("state file: array %r has dtype %s, not %s" % (name, a.dtype, dtype))
    if len(a.shape) != len(shape) or any(want is not None and want != have for want, have in zip(shape, a.shape)):
        raise ValueError("state file: array %r has shape %s, not %s" % (name, a.shape, tuple("n" if s is None else s for s in shape)))
    return a


def check_file(z):
    """every array of an opened state file (np.load(..., allow_pickle=False)), checked and returned as a dict; ValueError names the
    first array that is missing, of the wrong dtype or shape, or at odds with another"""
    ver = _get(z, "format_version", _I8, ())
    if int(ver) != FORMAT_VERSION:
        raise ValueError("state file: array 'format_version' is %d, this build reads %d only" % (int(ver), FORMAT_VERSION))
    out = {"dims": _get(z, "dims", _I8, (len(DIM_NAMES),))}
    d = dict(zip(DIM_NAMES, (int(x) for x in out["dims"])))
    neg = [k for k, v in d.items() if v < 0]
    if neg:
        raise ValueError("state file: array 'dims' holds a negative %s" % neg[0])
    for name, (dtype, shape) in array_specs(out["dims"]).items():
        out[name] = _get(z, "map_" + name, dtype, shape)
    for name, (dtype, shape) in host_specs(out).items():
        out[name] = _get(z, name, dtype, shape)

    def bad(name, why):
        raise ValueError("state file: array %r %s" % (name, why))
    # the rules of csrc/snapshot.h that the shapes do not already hold, in its order (the library checks them again on import)
    i32 = 2 ** 31 - 1
    if d["n_pts"] > i32 // 2 or d["n_obs"] > i32 // 2 or d["list_ids"] > i32 // 2 or d["kf_rows"] > i32 or d["kf_stored"] > i32 or d["id_bound"] > i32 + 1:
        bad("dims", "holds a count beyond int32 indexing")
    if d["img_cur"] not in (0, 1):
        bad("dims", "holds an img_cur that is not 0 or 1")
    for i in (0, 1):
        w, h, ch = d["img_w%d" % i], d["img_h%d" % i], d["img_ch%d" % i]
        if ch not in (0, 1, 3) or (w * h > 0 and ch == 0) or d["img_bytes%d" % i] != w * h * ch:
            bad("dims", "describes image %d with bytes that are not w * h * ch at 1 or 3 channels" % i)
    if not d["list_rows"] and d["list_ids"]:
        bad("dims", "holds list_ids without list_rows")
    if d["st_live0"] != d["n_pts"] or d["st_live1"] != d["n_obs"]:
        bad("dims", "holds st_live words that are not n_pts and n_obs")
    if len(out["id"]) and (out["id"].min() < 0 or out["id"].max() >= d["id_bound"]):
        bad("map_id", "holds an id outside [0, id_bound)")
    now = max(d["kf_stored"] - 1, 0)
    life = out["life"]
    if len(life) and ((life[:, :3] < 0).any() or (life[:, 2] > now).any()):
        bad("map_life", "holds a negative counter or a born beyond now")
    # the snapshot against its dims (the library checks every rule of csrc/snapshot.h again on import)
    if int(out["kf_cnt"].sum(dtype=np.int64)) != d["kf_rows"] or (out["kf_cnt"] < 0).any():
        bad("map_kf_cnt", "does not sum to dims' kf_rows")
    if out["obs_off"][0] != 0 or out["obs_off"][-1] != d["n_obs"] or (np.diff(out["obs_off"]) < 0).any():
        bad("map_obs_off", "does not run from 0 to dims' n_obs")
    if d["list_rows"] and (out["list_off"][0] != 0 or out["list_off"][-1] != d["list_ids"] or (np.diff(out["list_off"]) < 0).any()):
        bad("map_list_off", "does not run from 0 to dims' list_ids")
    if len(out["kf_ord"]) and (out["kf_ord"].max() >= d["kf_stored"] or (np.diff(out["kf_ord"]) <= 0).any() or out["kf_ord"].min() < 0):
        bad("map_kf_ord", "does not increase strictly below dims' kf_stored")
    # the host's bookkeeping against the snapshot
    n_rec = len(out["rec_n"])
    if n_rec < d["kf_stored"]:
        bad("rec_n", "holds fewer records than dims' kf_stored")
    if (out["rec_n"][out["kf_ord"]] != out["kf_cnt"]).any():
        bad("rec_n", "disagrees with map_kf_cnt at map_kf_ord")
    if len(out["dead_ref"]) != len(out["dead_desc"]):
        bad("dead_desc", "has not one row per row of dead_ref")
    ref = out["dref_kf"]
    if len(ref) and ref.max() >= n_rec:
        bad("map_dref_kf", "names a record beyond rec_n")
    live = np.zeros(n_rec + 1, bool)
    live[out["kf_ord"]] = True
    have = set(map(tuple, out["dead_ref"].tolist()))
    need = np.stack([ref, out["dref_row"]], 1)[(ref >= 0) & ~live[np.clip(ref, 0, n_rec)]] if len(ref) else np.zeros((0, 2), np.int64)
    if any(tuple(r) not in have for r in need.tolist()):
        bad("dead_ref", "lacks a descriptor row that map_dref_kf names in a removed keyframe")
    alive_rows = (ref >= 0) & live[np.clip(ref, 0, n_rec)] if len(ref) else np.zeros(0, bool)
    if alive_rows.any() and ((out["dref_row"][alive_rows] < 0) | (out["dref_row"][alive_rows] >= out["rec_n"][ref[alive_rows]])).any():
        bad("map_dref_row", "names a row its keyframe does not have")
    nj = len(out["inj_index"])
    for name in ("inj_id", "inj_pos", "inj_flags", "inj_color", "inj_desc"):
        if len(out[name]) != nj:
            bad(name, "has not one row per entry of inj_index")
    if len(out["inj_obs_off"]) != nj + 1 or out["inj_obs_off"][0] != 0 or out["inj_obs_off"][-1] != len(out["inj_obs"]) or \
            (np.diff(out["inj_obs_off"]) < 0).any():
        bad("inj_obs_off", "does not run from 0 to the rows of inj_obs")
    n_inj = int(out["n_injected"])
    if nj and (out["inj_index"].min() < 0 or out["inj_index"].max() >= n_inj or len(np.unique(out["inj_index"])) != nj):
        bad("inj_index", "does not name distinct entries below n_injected")
    if len(ref) and (-ref[ref < 0] - 1 >= n_inj).any():
        bad("map_dref_kf", "names an injected point beyond n_injected")
    if len(ref) and not set((-ref[ref < 0] - 1).tolist()) <= set(out["inj_index"].tolist()):
        bad("inj_index", "lacks an injected point that map_dref_kf names")
    if len(out["lc_off"]) != len(out["lc_counts"]) + 1 or out["lc_off"][0] != 0 or out["lc_off"][-1] != len(out["lc_serials"]) or \
            (np.diff(out["lc_off"]) < 0).any():
        bad("lc_off", "does not run from 0 to the length of lc_serials")
    if len(out["vocab_words"]) != len(out["vocab_weights"]):
        bad("vocab_weights", "has not one weight per row of vocab_words")
    if (out["list_rows"] >= max(d["list_rows"], 1)).any() or (out["list_rows"] < -1).any():
        bad("list_rows", "names a row beyond dims' list_rows")
    if (out["covis"][:, 2] < 0).any():
        bad("covis", "holds a negative count")
    n_kf = d["n_kf"]
    shapes = out["image_shapes"]
    if len(shapes) != (n_kf if int(out["images_all"]) else 0):
        bad("image_shapes", "has not one row per keyframe of a file saved with images='all'")
    for k, (h, w, ch) in enumerate(shapes.tolist()):
        if h < 0 or w < 0 or ch not in (0, 1, 3):
            bad("image_shapes", "holds a shape that is no image")
        out["kf_image_%d" % k] = _get(z, "kf_image_%d" % k, _U1, (h, w) if ch == 0 else (h, w, ch))
    if "last_image" not in z.files:
        raise ValueError("state file: array 'last_image' is missing")
    try:
        last = z["last_image"]
    except ValueError as e:
        raise ValueError("state file: array 'last_image' cannot be read without pickle (%s)" % e) from None
    if last.dtype != _U1 or last.ndim not in (2, 3) or (last.ndim == 3 and last.shape[2] not in (1, 3)):
        bad("last_image", "is no uint8 image")
    if last.size and tuple(out["last_image_size"].tolist()) != last.shape[1::-1]:
        bad("last_image_size", "is not the size of last_image")
    if (out["last_image_size"] < 0).any():
        bad("last_image_size", "holds a negative size")
    out["last_image"] = last
    return out
