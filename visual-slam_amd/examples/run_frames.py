#!/usr/bin/env python3
"""Frame loop in the style of the reference's src/tests/tester_map.py:32-110 / src/run_video.py:64-71,140-152, driven by the
drop-in classes only.

The reference's Tracker / LocalMapper are not part of this repo; this small state machine reproduces the calls Tracker makes on
the three classes (tracker.py:87,162,168-170,214,221,230,242-249):
    NOT_INITIALIZED: frame 0 -> set_first_frame, frame 1.. -> initialize (two-view map)
    TRACKING: match against the previous frame, the two match filters (threshold_percent = 0.02, tracker.py:219), essential matrix
              at threshold 1.0 + pose - as one fused device call (orbslam2.utils.track_from_last_frame, default) or with the filters
              as Python loops over DMatch objects like the reference (--python-filters)

Inputs:
    --config <yaml>   the reference's configuration file (configs/monocular.yaml): camera.camera_matrix (9 floats, row-major),
                      camera.distortion_coeffs (k1 k2 p1 p2 k3), orb.n_features / scale_factor / n_levels / ini_threshold /
                      min_threshold, matcher.matcher_type / ratio_threshold, skip_frames, max_frames.  Without it: the values of
                      configs/monocular.yaml:3,8-12 with the Tracker's ratio 0.75.
    --frames <path>   a directory of image files (sorted by name; anything PIL opens), or a .npy / .npz array [N, H, W] or
                      [N, H, W, 3] (BGR like cv2).  Frames are undistorted on the device when a distortion coefficient is non-zero
                      (run_video.py:145-149) and converted to gray on the device.  Without it: a synthetic sequence (a camera
                      translating past a two-depth scene), so the drop-in can be exercised end to end without cv2 or a video file.
    --batch N         the same sequence through vslam_amd.stream.FrameStream: frames are gathered into chunks of N and every chunk is
                      ONE batched device call (upload of the next chunk and the handling of the previous one overlapped with the
                      compute); the first two frames still initialise the map through MapInitializer, every later frame takes its
                      tracking result (against the previous frame) from the stream.  Same keypoints, descriptors, kept matches and
                      poses as the per-frame loop - at the batched mode's rate.
    --load-state FILE --localize [--batch N] [--reloc-preselect P]
                      localise every frame of the input in the saved map: no tracking, no initialisation, the map is not extended.
                      Without --batch every frame is extracted and relocalised on its own (LocalMapper.relocalize); with --batch N the
                      extraction runs through FrameStream and every chunk of N frames is ONE LocalMapper.relocalize_batch, fed with the
                      chunk's keypoint and descriptor arrays.  One line per frame: ok, keyframe id, inliers, pose - the same lines
                      either way.
Usage: python visual-slam_amd/examples/run_frames.py [--config cfg.yaml] [--frames dir|file] [--max-frames 30] [--grid] [--python-filters] [--batch 64]
       [--map PATH [--relocalize [--vocabulary PATH [--reloc-preselect N]]] [--vocabulary PATH --detect-loops [--loop-sim3 [--loop-confirm [--loop-correct [--loop-optimize [--loop-global-ba]]]]]] [--track-map [--vocabulary PATH --track-reference] [--covisible] [--grow-neighbours] [--fuse] [--local-ba [--ba-window 10] [--ba-covisible] [--ba-erase-outliers]] [--cull-points]] [--cull-keyframes] [--save-state FILE] [--load-state FILE] [--merge-into FILE]]
       [--load-state FILE --localize [--batch N] [--vocabulary PATH --reloc-preselect P]]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from orbslam2 import utils as geom                      # noqa: E402
from orbslam2.extractor import ORBExtractor             # noqa: E402
from orbslam2.initializer import MapInitializer         # noqa: E402
from orbslam2.matcher import DescriptorMatcher          # noqa: E402

W, H = 640, 480
DEFAULTS = {"camera": {"camera_matrix": [320.0, 0.0, 320.0, 0.0, 320.0, 240.0, 0.0, 0.0, 1.0], "distortion_coeffs": [0.0] * 5},
            "orb": {"n_features": 2000, "scale_factor": 1.2, "n_levels": 8, "ini_threshold": 20, "min_threshold": 7},
            "matcher": {"matcher_type": "bruteforce-hamming", "ratio_threshold": 0.75}, "skip_frames": 0, "max_frames": 0}


def load_config(path):
    """the reference's utils.load_config + load_camera_intrinsics (utils.py:6-37) -> (config dict with defaults filled in, K 3x3, D)"""
    import yaml
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULTS.items()}
    if path:
        with open(path) as f:
            user = yaml.safe_load(f) or {}
        ucam = user.get("camera", {}) or {}
        if "camera_matrix" not in ucam or "distortion_coeffs" not in ucam:   # utils.py:31-32 of the reference
            raise KeyError("'camera_matrix' or 'distortion_coeffs' missing in 'camera' section of config")
        for k, v in user.items():
            if isinstance(v, dict) and isinstance(cfg.get(k), dict):
                cfg[k].update(v)
            else:
                cfg[k] = v
    cam = cfg["camera"]
    K = np.array(cam["camera_matrix"], dtype=float).reshape(3, 3)
    D = np.array(cam["distortion_coeffs"], dtype=float)
    return cfg, K, D


def scene(seed, w, h, rects):
    rng = np.random.Generator(np.random.PCG64(seed))
    img = np.full((h, w), 128.0) + 25 * np.sin(np.arange(w) / 47.0)[None, :] + 25 * np.cos(np.arange(h) / 31.0)[:, None]
    for _ in range(rects):
        rw, rh = rng.integers(5, 22, size=2)
        x, y = rng.integers(0, w - 1), rng.integers(0, h - 1)
        img[y:y + rh, x:x + rw] = rng.uniform(0, 255)
    return np.clip(img + rng.normal(0, 1, img.shape), 0, 255)


def synthetic_sequence(n, seed=7):
    """a camera translating along x past two depth layers: the background pans 4 px / frame, the foreground patches 8 px / frame
    (both inside the tracker's displacement gate of 2 % of (w + h) / 2 = 11.2 px, tracker.py:219)"""
    span = 8 * n + W
    bg, fg, mk = scene(seed, span, H, 800 * span // W), scene(seed + 1, span, H, 800 * span // W), scene(seed + 2, span, H, 40 * span // W)
    rng = np.random.default_rng(seed)
    for i in range(n):
        fr = np.where(mk[:, 8 * i:8 * i + W] > 130, fg[:, 8 * i:8 * i + W], bg[:, 4 * i:4 * i + W])
        yield np.clip(np.rint(fr + rng.normal(0, 1, fr.shape)), 0, 255).astype(np.uint8)


def frames_from(path):
    """a directory of images (BGR arrays like cv2.imread, in name order) or a .npy / .npz stack"""
    if os.path.isdir(path):
        from PIL import Image
        for name in sorted(os.listdir(path)):
            try:
                im = Image.open(os.path.join(path, name))
            except Exception:
                continue  # not an image (e.g. gt.yaml beside the frames)
            a = np.array(im.convert("RGB") if im.mode not in ("L", "I;16") else im.convert("L"))
            yield np.ascontiguousarray(a[:, :, ::-1]) if a.ndim == 3 else a
        return
    data = np.load(path)
    arr = data[sorted(data.files)[0]] if hasattr(data, "files") else data
    for a in arr:
        yield np.ascontiguousarray(a, dtype=np.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="", help="YAML file with the reference's keys (configs/monocular.yaml)")
    ap.add_argument("--frames", default="", help="directory of images, or .npy / .npz frame stack; default: synthetic sequence")
    ap.add_argument("--max-frames", type=int, default=30, help="frames of the synthetic sequence / cap on the input (0 = config's max_frames)")
    ap.add_argument("--grid", action="store_true", help="extract_features(distributed=True), the path Tracker.process_frame takes")
    ap.add_argument("--python-filters", action="store_true", help="tracking step through the per-method API (Python filter loops)")
    ap.add_argument("--map", default="", help="PATH: keyframes into the device LocalMapper (vslam_amd.mapper), its PLY map written to PATH")
    ap.add_argument("--keyframe-every", type=int, default=20, help="with --map: a keyframe every N frames (tracker.py:290)")
    ap.add_argument("--relocalize", action="store_true", help="with --map: when the tracking step fails, relocalize the frame against the "
                    "device map (LocalMapper.relocalize) and go on tracking from it")
    ap.add_argument("--vocabulary", default="", help="with --map --relocalize: PATH of a place-recognition vocabulary (.npz of vslam_amd.Vocabulary.save) "
                    "attached to the map; a file that does not exist is trained from the map's keyframes (up to 1024 words) at the first "
                    "relocalization and saved there")
    ap.add_argument("--reloc-preselect", type=int, default=0, help="with --vocabulary: N > 0: relocalize matches the frame only against the N "
                    "keyframes the vocabulary query ranks first (LocalMapper.relocalize(preselect=N))")
    ap.add_argument("--track-reference", action="store_true", help="with --map --track-map --vocabulary: when the search by projection fails, "
                    "the frame is tracked against the last keyframe by appearance (LocalMapper.track_reference_keyframe) and the local map is "
                    "tracked from that pose; the essential-matrix step and --relocalize come only after that")
    ap.add_argument("--detect-loops", action="store_true", help="with --map --vocabulary: after each keyframe, look for a loop (LocalMapper.detect_loop: "
                    "place-recognition candidates on the covisibility graph, three consistent detections in a row, map-point matches); one "
                    "line per keyframe with candidates, one when a loop is found")
    ap.add_argument("--loop-sim3", action="store_true", help="with --detect-loops: a loop is found only when the candidate also aligns with the "
                    "keyframe by a similarity (LocalMapper.detect_loop(sim3=True): 3-point RANSAC and refinement on the matched map points); "
                    "the line of a found loop then carries the relative scale and the inlier count")
    ap.add_argument("--loop-confirm", action="store_true", help="with --detect-loops (switches --loop-sim3 on): an aligned candidate is accepted only "
                    "when the guided search, the refit and the projection of its neighbourhood (LocalMapper.detect_loop(sim3=True, confirm=True)) "
                    "give 40 loop points; the line of a found loop then carries their number and the split by source")
    ap.add_argument("--loop-correct", action="store_true", help="with --detect-loops (switches --loop-confirm and --loop-sim3 on): a confirmed loop is "
                    "corrected (LocalMapper.detect_loop(..., correct=True)): the keyframe's neighbourhood and its points move onto the old side and the "
                    "duplicates across the loop are fused; the line of a found loop then carries the counts")
    ap.add_argument("--loop-optimize", action="store_true", help="with --detect-loops (switches --loop-correct on): the essential graph is optimised "
                    "behind the correction (LocalMapper.detect_loop(..., optimize=True)): a Sim(3) pose graph over all keyframes spreads what the "
                    "correction left along the trajectory; the line of a found loop then carries the cost before and after")
    ap.add_argument("--loop-global-ba", action="store_true", help="with --detect-loops (switches --loop-optimize on): a global bundle adjustment runs "
                    "behind the essential graph (LocalMapper.detect_loop(..., global_ba=True)): every keyframe but the first and every point with two "
                    "observations; the line of a found loop then carries its cost before and after")
    ap.add_argument("--track-map", action="store_true", help="with --map: track every frame against the device map from the constant-velocity "
                    "prediction (LocalMapper.track_local_map); the essential-matrix step runs only when that fails")
    ap.add_argument("--covisible", action="store_true", help="with --map --track-map: the local map of a frame is what the covisible keyframes "
                    "see (track_local_map(local=\"covisible\"): the keyframes observing the points the previous frame matched, and their best "
                    "covisible neighbours) instead of what the last 10 keyframes see")
    ap.add_argument("--frustum", action="store_true", help="with --map --track-map (and --fuse): search by projection under ORB-SLAM2's frustum "
                    "test and predicted pyramid level (track_local_map / fuse_map_points with frustum=True) with the extractor's levels and scale factor")
    ap.add_argument("--local-ba", action="store_true", help="with --map --track-map: a tracked frame that becomes a keyframe hands its matches to "
                    "the map (add_keyframe(tracked=)), and local bundle adjustment (LocalMapper.bundle_adjust) runs after it")
    ap.add_argument("--fuse", action="store_true", help="with --map --track-map: after each keyframe added from a tracked frame, duplicate map points "
                    "are merged and missing observations gained (LocalMapper.fuse_map_points), before the bundle adjustment of --local-ba")
    ap.add_argument("--grow-neighbours", action="store_true", help="with --map --track-map: after each keyframe added from a tracked frame, its "
                    "keypoints without a map point are searched along their epipolar lines in the neighbour keyframes and triangulated "
                    "(LocalMapper.create_new_map_points with its default window of 10 neighbours), before --fuse and the bundle adjustment of --local-ba")
    ap.add_argument("--cull-keyframes", action="store_true", help="with --map: after each keyframe's mapping steps, ORB-SLAM2's KeyFrameCulling asked "
                    "from the new keyframe (LocalMapper.cull_keyframes: decided and erased on the device); the reference's own keyframe cull is "
                    "switched off (redundancy_threshold = inf), since it leaves stale observation keys behind")
    ap.add_argument("--cull-points", action="store_true", help="with --map --track-map: every tracked frame is recorded in the map points' found / "
                    "visible counters (LocalMapper.note_tracking, with the frame's local map and --frustum setting), and after each keyframe's "
                    "mapping steps ORB-SLAM2's MapPointCulling removes the bad points (LocalMapper.cull_map_points), before --cull-keyframes; use it with "
                    "--cull-keyframes: the reference's own keyframe cull leaves stale observation keys, which its map-point cull then raises on")
    ap.add_argument("--ba-window", type=int, default=10, help="with --local-ba: keyframes the bundle adjustment frees, counted from the last (at most 16)")
    ap.add_argument("--ba-covisible", action="store_true", help="with --local-ba: the bundle adjustment frees the new keyframe and its covisible "
                    "neighbours (LocalMapper.bundle_adjust(local=\"covisible\"): at most 15 keyframes sharing 15 points with it), not the last --ba-window")
    ap.add_argument("--ba-erase-outliers", action="store_true", help="with --local-ba: the observations a bundle adjustment ends with as outliers are "
                    "erased from the map on the device (LocalMapper.bundle_adjust(erase_outliers=True)); with --cull-points the cull that follows "
                    "removes the points left under-observed")
    ap.add_argument("--save-state", default="", help="with --map: FILE the whole mapper is written to at the end (LocalMapper.save_state: the device "
                    "map's snapshot, the keyframes, the vocabulary), to localise in later with --load-state")
    ap.add_argument("--load-state", default="", help="with --map: start from the mapper saved in FILE (LocalMapper.load_state) instead of initialising; "
                    "with --relocalize or --track-map the first frame is relocalised against it, otherwise tracking goes on from its last keyframe's pose")
    ap.add_argument("--merge-into", default="", help="with --map: at the end of the run FILE (a mapper saved by --save-state) is loaded as the base and "
                    "the run's map is merged into it (LocalMapper.merge_map: absorbed on the device, aligned by the loop calls; the base's vocabulary "
                    "is used, else --vocabulary's); --save-state then writes the merged mapper")
    ap.add_argument("--init-model-selection", action="store_true", help="initialise with ORB-SLAM2's homography / fundamental model selection "
                    "(MapInitializer(model_selection=True)): prints model, RH, parallax and good counts of every attempt")
    ap.add_argument("--batch", type=int, default=0, help="N > 0: the sequence through FrameStream in chunks of N frames (one batched device call each)")
    ap.add_argument("--localize", action="store_true", help="with --load-state: every frame of the input is relocalised in the saved map, which is "
                    "not extended; with --batch N one LocalMapper.relocalize_batch per chunk of N frames")
    args = ap.parse_args(argv)
    cfg, K, D = load_config(args.config)
    orb, mt = cfg["orb"], cfg["matcher"]
    extractor = ORBExtractor(n_features=orb["n_features"], scale_factor=orb["scale_factor"], n_levels=orb["n_levels"],
                             ini_threshold=orb["ini_threshold"], min_threshold=orb["min_threshold"])
    matcher = DescriptorMatcher(mt["matcher_type"], ratio_threshold=mt["ratio_threshold"])
    initializer = MapInitializer(K, model_selection=args.init_model_selection)
    limit = args.max_frames or cfg.get("max_frames", 0) or 10 ** 9
    skip = int(cfg.get("skip_frames", 0) or 0)
    source = frames_from(args.frames) if args.frames else synthetic_sequence(limit if limit < 10 ** 9 else 30)
    state, last, poses, n_map, n_seen = "NOT_INITIALIZED", None, [], 0, 0
    t0 = time.perf_counter()
    if args.localize:
        if not args.load_state:
            ap.error("--localize needs --load-state")
        if args.reloc_preselect < 0:
            ap.error("--reloc-preselect must be >= 0")
        return run_localize(args, K, D, orb, extractor, source, limit, skip, t0)
    if args.batch > 0:
        if args.map:
            ap.error("--map runs frame by frame: it cannot be combined with --batch")
        return run_batched(args, cfg, K, D, orb, mt, initializer, source, limit, skip, t0)
    if args.relocalize and not args.map:
        ap.error("--relocalize needs --map")
    if (args.save_state or args.load_state) and not args.map:
        ap.error("--save-state and --load-state need --map")
    if args.merge_into and not args.map:
        ap.error("--merge-into needs --map")
    if args.vocabulary and not ((args.relocalize or args.detect_loops or args.track_reference or args.merge_into) and args.map):
        ap.error("--vocabulary needs --map and --relocalize, --detect-loops, --track-reference or --merge-into")
    if args.track_reference and not (args.map and args.track_map and args.vocabulary):
        ap.error("--track-reference needs --map, --track-map and --vocabulary")
    if args.detect_loops and not args.vocabulary:
        ap.error("--detect-loops needs --map and --vocabulary")
    if args.loop_global_ba and not args.detect_loops:
        ap.error("--loop-global-ba needs --detect-loops")
    args.loop_optimize = args.loop_optimize or args.loop_global_ba
    if args.loop_optimize and not args.detect_loops:
        ap.error("--loop-optimize needs --detect-loops")
    args.loop_correct = args.loop_correct or args.loop_optimize
    if args.loop_correct and not args.detect_loops:
        ap.error("--loop-correct needs --detect-loops")
    args.loop_confirm = args.loop_confirm or args.loop_correct
    if args.loop_confirm and not args.detect_loops:
        ap.error("--loop-confirm needs --detect-loops")
    args.loop_sim3 = args.loop_sim3 or args.loop_confirm
    if args.loop_sim3 and not args.detect_loops:
        ap.error("--loop-sim3 needs --detect-loops")
    if args.reloc_preselect and not args.vocabulary:
        ap.error("--reloc-preselect needs --vocabulary")
    if args.reloc_preselect < 0:
        ap.error("--reloc-preselect must be >= 0")
    if args.track_map and not args.map:
        ap.error("--track-map needs --map")
    if args.covisible and not args.track_map:
        ap.error("--covisible needs --map and --track-map")
    if args.local_ba and not args.track_map:
        ap.error("--local-ba needs --map and --track-map")
    if (args.ba_covisible or args.ba_erase_outliers) and not args.local_ba:
        ap.error("--ba-covisible and --ba-erase-outliers need --local-ba")
    if args.fuse and not args.track_map:
        ap.error("--fuse needs --map and --track-map")
    if args.cull_keyframes and not args.map:
        ap.error("--cull-keyframes needs --map")
    if args.grow_neighbours and not args.track_map:
        ap.error("--grow-neighbours needs --map and --track-map")
    if args.cull_points and not args.track_map:
        ap.error("--cull-points needs --map and --track-map")
    mapper, first, ref_pose = None, None, np.eye(4)
    n_ba = [0, 0]   # --local-ba: calls, calls that ended ok
    n_ba_erased = [0, 0]   # --ba-erase-outliers: entries erased, points left with fewer than two
    n_fuse = [0, 0, 0]   # --fuse: calls, points absorbed, observations gained
    n_cull = [0, 0]      # --cull-keyframes: calls, keyframes removed
    n_grow = [0, 0, 0]   # --grow-neighbours: calls, points created, their observations
    n_ptcull = [0, 0, 0, 0]   # --cull-points: frames noted, culls, points removed, points tested
    n_trackref = [0]   # --track-reference: frames it gave a pose
    recent = []   # --track-map: the last two poses, for the constant-velocity prediction
    n_loop = [0, 0]   # --detect-loops: calls, loops found
    seeds = [None]   # --covisible: the previous frame's matched map points (indices into the map as it stands: dropped when the map changes)
    if args.map:
        from vslam_amd.mapper import LocalMapper, predict_pose
        if args.load_state:   # localise in a saved map: no initialisation, the frames are tracked in its frame and scale
            mapper = LocalMapper.load_state(args.load_state, output_path=args.map)
            state = "TRACKING"
            if mapper.keyframes:
                ref_pose = mapper.keyframes[-1]["pose"].copy()
            print("loaded %s: %d keyframes, %d map points%s" % (args.load_state, len(mapper.keyframes), len(mapper.map_points),
                                                              ", vocabulary of %d words" % len(mapper.vocabulary) if mapper.vocabulary is not None else ""))
        else:
            mapper = LocalMapper(K, args.map)
        if args.cull_keyframes:
            mapper.redundancy_threshold = float("inf")
        if args.vocabulary and os.path.exists(args.vocabulary):
            import vslam_amd
            mapper.set_vocabulary(vslam_amd.Vocabulary.load(args.vocabulary, context=mapper.ctx))
            print("vocabulary: %d words from %s" % (len(mapper.vocabulary), args.vocabulary))

    def ensure_vocabulary(idx):
        """--vocabulary names a file that does not exist: trained from the map's keyframes at its first use and saved there"""
        if args.vocabulary and mapper.vocabulary is None and mapper.keyframes:
            rows = sum(len(kf["descriptors"]) for kf in mapper.keyframes)
            if rows >= 2:
                v = mapper.train_vocabulary(min(1024, rows))
                v.save(args.vocabulary)
                print("frame %d: vocabulary of %d words trained on %d rows of %d keyframes in %d iterations, saved to %s"
                      % (idx, len(v), rows, len(mapper.keyframes), v.iterations, args.vocabulary))

    def detect_loop(idx):
        """--detect-loops, after a keyframe was added (ORB-SLAM2's LoopClosing::DetectLoop up to the point correspondences)"""
        if not args.detect_loops:
            return
        ensure_vocabulary(idx)
        if mapper.vocabulary is None:
            return
        found, info = mapper.detect_loop(sim3=args.loop_sim3, confirm=args.loop_confirm, correct=args.loop_correct, optimize=args.loop_optimize,
                                          global_ba=args.loop_global_ba)
        n_loop[0] += 1
        if info["candidates"]:
            print("frame %d: keyframe %d loop candidates %s" % (idx, info["kf_pos"], ", ".join(
                "%d (score %.3f, group score %.3f, consistency %d, %d matches)" % (c["pos"], c["score"], c["acc"], c["consistency"], c["n_match"])
                for c in info["candidates"])))
        if found:
            n_loop[1] += 1
            acc = info["accepted"]
            confirmed = ""
            if args.loop_confirm:
                cf = acc["confirm"]
                by = [int((cf["source"] == k).sum()) for k in (1, 2, 3)]
                confirmed = "; confirmed by %d loop points (%d seeds, %d guided, %d projected)" % (cf["n_total"], by[0], by[1], by[2])
            if args.loop_correct:
                co = acc["correct"]
                confirmed += "; corrected %d keyframes and %d points by scale %.4f, %d points fused away, %d observations gained, %d new connections" % (
                    co["n_corrected"], co["n_moved"], co["A_scale"], co["n_absorbed"], co["n_direct_gained"] + co["n_gained"],
                    sum(len(v) for v in co["loop_connections"].values()))
                seeds[0] = None   # (map point indices changed)
            if args.loop_optimize:
                og = acc["optimize"]
                confirmed += "; essential graph of %d edges over %d free keyframes optimised in %d steps (%d accepted, %d solver iterations): cost %.6g -> %.6g, %d points followed" % (
                    og["n_edges"], og["n_free"], og["steps"], og["accepted"], og["cg_iters"], og["cost"][0], og["cost"][1], og["n_moved"])
            if args.loop_global_ba:
                gb = acc["global_ba"]
                confirmed += "; global bundle adjustment of %d free keyframes, %d points and %d edges in %d steps (%d accepted, %d solver iterations): cost %.6g -> %.6g, %d inlier edges" % (
                    gb["n_free"], gb["n_points"], gb["n_edges"], gb["steps"], gb["accepted"], gb["cg_iters"], gb["cost"][0], gb["cost"][1], gb["n_inliers"])
            print("frame %d: loop found: keyframe %d closes with keyframe %d, %d map-point correspondences%s%s"
                  % (idx, info["kf_pos"], acc["pos"], acc["n_match"],
                     ", relative scale %.4f with %d inliers" % (acc["sim3"]["scale"], acc["sim3"]["n_inliers"]) if args.loop_sim3 else "", confirmed))

    def track_pose(R, t, frame, kps, desc, idx):
        """Tracker._update_pose (tracker.py:268-279) and the keyframe every N frames (tracker.py:114-118, 290)"""
        nonlocal ref_pose
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = np.asarray(t).reshape(3)
        ref_pose = ref_pose @ T
        recent[:] = recent[-1:] + [ref_pose]
        if mapper is not None and idx % args.keyframe_every == 0:
            mapper.add_keyframe(frame, kps, desc, ref_pose)
            cull(idx)
            detect_loop(idx)

    frustum_kw = {"frustum": True, "n_levels": int(orb["n_levels"]), "scale_factor": float(orb["scale_factor"])} if args.frustum else {}

    def fuse(idx):
        fi = mapper.fuse_map_points(window=args.ba_window, **frustum_kw)
        n_fuse[0] += 1
        n_fuse[1] += fi["n_absorbed"]
        n_fuse[2] += fi["n_gained"]
        print("frame %d: fuse %d absorbed, %d gained (%d proposals of %d candidates), %d map points"
              % (idx, fi["n_absorbed"], fi["n_gained"], fi["n_proposals"], fi["n_cand"], fi["n_points"]))

    def cull(idx):
        if args.cull_points:
            removed, pi = mapper.cull_map_points()
            n_ptcull[1] += 1
            n_ptcull[2] += len(removed)
            n_ptcull[3] += pi["n_tested"]
            print("frame %d: point cull removed %d of %d tested (found ratio %d, observations %d, orphans %d), %d map points, %d observations"
                  % (idx, len(removed), pi["n_tested"], pi["n_reason"][1], pi["n_reason"][2], pi["n_reason"][3], pi["n_points"], pi["n_obs"]))
        if not args.cull_keyframes:
            return
        removed, ci = mapper.cull_keyframes()
        n_cull[0] += 1
        n_cull[1] += len(removed)
        print("frame %d: keyframe cull removed %s of %d candidates (redundant points %s of %s), %d keyframes, %d observations"
              % (idx, removed, ci["n_local"], ci["n_redundant"].tolist(), ci["n_points"].tolist(), len(mapper.keyframes), ci["n_obs"]))

    def grow(idx):
        gi = mapper.create_new_map_points()   # (its own window of 10 neighbours; --ba-window belongs to --local-ba and --fuse)
        n_grow[0] += 1
        n_grow[1] += gi["n_new"]
        n_grow[2] += gi["n_obs_new"]
        print("frame %d: grow %d new points with %d observations (%d matches of %d free rows, %d neighbours), %d map points"
              % (idx, gi["n_new"], gi["n_obs_new"], gi["n_matches"], gi["n_free"], gi["n_neighbours"], gi["n_points"]))

    def track_map(frame, kps, desc, idx):
        """the frame against the device map from the predicted pose (ORB-SLAM2's TrackWithMotionModel + TrackLocalMap); on success its
        pose becomes the reference pose"""
        nonlocal ref_pose
        pred = predict_pose(recent[-2], recent[-1]) if len(recent) >= 2 else ref_pose
        if args.covisible:
            ok, T, info = mapper.track_local_map(kps, desc, pred, local="covisible", seed_points=seeds[0], **frustum_kw)
            seeds[0] = info["point"] if ok else None
        else:
            ok, T, info = mapper.track_local_map(kps, desc, pred, **frustum_kw)
        if not ok and args.track_reference:   # ORB-SLAM2's TrackReferenceKeyFrame: the last keyframe by appearance, then the local map from its pose
            ensure_vocabulary(idx)
            if mapper.vocabulary is not None:
                rok, rT, rinfo = mapper.track_reference_keyframe(kps, desc)
                print("frame %d: track reference keyframe %s, %d candidates, %d matches (%d before the orientation check), %d inliers"
                      % (idx, "ok" if rok else "failed", rinfo["n_cand"], rinfo["n_matches"], rinfo["n_matches_raw"], rinfo["n_inliers"]))
                if rok:
                    n_trackref[0] += 1
                    if args.covisible:
                        ok, T, info = mapper.track_local_map(kps, desc, rT, local="covisible", seed_points=rinfo["point"], **frustum_kw)
                        seeds[0] = info["point"] if ok else None
                    else:
                        ok, T, info = mapper.track_local_map(kps, desc, rT, **frustum_kw)
        if idx % 5 == 0:
            print("frame %d: track map %s, %d matches, %d inliers, t = %s" % (idx, "ok" if ok else "failed", info["pass_matches"][-1] if
                  info["n_pass_run"] else 0, info["pass_inliers"][-1] if info["n_pass_run"] else 0, np.round(T[:3, 3], 3)))
        if ok:
            if args.cull_points:   # (before the keyframe below changes the map the matches index)
                mapper.note_tracking(T, info, **frustum_kw)
                n_ptcull[0] += 1
            ref_pose = T
            recent[:] = recent[-1:] + [T]
            poses.append((T[:3, :3], T[:3, 3:4]))
            if idx % args.keyframe_every == 0:
                seeds[0] = None   # (the cull and the fusion below renumber the map points)
                if args.local_ba:
                    mapper.add_keyframe(frame, kps, desc, T, tracked=(info["point"], info["inlier"]))
                    if args.grow_neighbours:
                        grow(idx)
                    if args.fuse:
                        fuse(idx)
                    if args.ba_covisible or args.ba_erase_outliers:
                        ba_ok, ba = mapper.bundle_adjust(window=args.ba_window, local="covisible" if args.ba_covisible else "window",
                                                         erase_outliers=args.ba_erase_outliers)
                    else:
                        ba_ok, ba = mapper.bundle_adjust(window=args.ba_window)
                    n_ba[0] += 1
                    n_ba[1] += ba_ok
                    print("frame %d: bundle adjust %s, %d free + %d fixed keyframes, %d points, %d of %d edges inliers, cost %.4g -> %.4g, steps %s"
                          % (idx, "ok" if ba_ok else "not ok", ba["n_free"], ba["n_fixed"], ba["n_local"], ba["n_inliers"], ba["n_edges"],
                             ba["cost"][0], ba["cost"][2], ba["steps"]))
                    if args.ba_covisible or args.ba_erase_outliers:
                        n_ba_erased[0] += ba["n_erased"]
                        n_ba_erased[1] += ba["n_under"]
                        print("frame %d: bundle adjust over the keyframes %s, %d outlier observations erased, %d points left with fewer than two"
                              % (idx, ba["candidates"], ba["n_erased"], ba["n_under"]))
                    if ba["n_free"] and mapper.keyframes[-1]["descriptors"] is desc:   # tracking goes on from the refined pose of this keyframe
                        T = mapper.keyframes[-1]["pose"].copy()
                        ref_pose = T
                        recent[-1] = T
                else:
                    mapper.add_keyframe(frame, kps, desc, T)
                    if args.grow_neighbours:
                        grow(idx)
                    if args.fuse:
                        fuse(idx)
                cull(idx)
                detect_loop(idx)
        return ok

    def relocalize(frame, kps, desc, idx):
        """the frame against the map (ORB-SLAM2's Tracking::Relocalization); on success tracking goes on from its pose"""
        nonlocal ref_pose
        ensure_vocabulary(idx)
        pre = args.reloc_preselect if args.reloc_preselect > 0 and mapper.vocabulary is not None else None
        ok, T, info = mapper.relocalize(kps, desc, preselect=pre)
        print("frame %d: relocalize %s, keyframe %s, %d candidates, %d inliers%s" % (idx, "ok" if ok else "failed", info["kf_pos"],
                                                                                    len(info["candidates"]), info["n_inliers"],
                                                                                    "" if pre is None else " (preselect %d)" % pre))
        if ok:
            ref_pose = T
            recent[:] = recent[-1:] + [T]
            poses.append((T[:3, :3], T[:3, 3:4]))
    for idx, frame in enumerate(source):
        if n_seen >= limit:
            break
        if skip and idx % (skip + 1) != 0:   # tester_map.py:60-63
            continue
        n_seen += 1
        if np.any(D):                        # run_video.py:145-149
            frame = geom.undistort_image(frame, K, D)
        if args.grid:                        # Tracker's default path; keypoint i belongs to descriptor row i (see distribute_keypoints)
            kps, desc = extractor.distribute_keypoints(frame, aligned=True)
        else:
            kps, desc = extractor.extract_features(frame, distributed=False)
        if args.load_state and last is None:   # the first frame against a loaded map
            if args.relocalize or args.track_map:
                relocalize(frame, kps, desc, idx)
        elif state == "NOT_INITIALIZED":
            if initializer.first_frame_keypoints is None:
                initializer.set_first_frame(kps, desc, frame)
                first = (frame, kps, desc)
            else:
                ok, R, t, pts, matches = initializer.initialize(kps, desc, matcher, frame)
                _print_selection(idx, initializer)
                if ok:
                    state, n_map = "TRACKING", len(pts)
                    poses.append((R, t))
                    print("frame %d: initialised, %d map points, t = %s" % (idx, n_map, np.round(t.ravel(), 3)))
                    if mapper is not None:   # tracker.py:172-189: both frames as keyframes, then the initial map points
                        T = np.eye(4)
                        T[:3, :3] = R
                        T[:3, 3] = np.asarray(t).reshape(3)
                        mapper.add_keyframe(first[0], first[1], first[2], ref_pose)
                        mapper.add_keyframe(frame, kps, desc, T)
                        mapper.update_map_points([p for p in pts if isinstance(p, dict)])
                        if args.track_map:   # tracking goes on in the map's frame: from the second keyframe's pose
                            ref_pose = T
                            recent[:] = [np.eye(4), T]
        elif args.track_map and track_map(frame, kps, desc, idx):
            pass
        elif not args.python_filters:
            ok, T, inl = geom.track_from_last_frame(last[0], last[1], kps, desc, K, frame.shape, ratio_threshold=mt["ratio_threshold"],
                                                    threshold_percent=0.02)   # tracker.py:219
            if ok:
                poses.append((T[:3, :3], T[:3, 3:4]))
                track_pose(T[:3, :3], T[:3, 3], frame, kps, desc, idx)
                if idx % 5 == 0:
                    print("frame %d: %d pose inliers, t = %s" % (idx, len(inl), np.round(T[:3, 3], 3)))
            elif args.relocalize:
                relocalize(frame, kps, desc, idx)
        else:
            m = matcher.match(last[1], desc)
            m = matcher.filter_matches_by_geometric_distance(last[0], kps, m, 0.02, frame.shape)   # tracker.py:219-221
            m = matcher.filter_matches_by_distance(m)
            if len(m) >= 8:
                p1 = np.float32([last[0][x.queryIdx].pt for x in m])
                p2 = np.float32([kps[x.trainIdx].pt for x in m])
                E, mask = geom.calculate_essential_matrix(p1, p2, K, prob=0.999, threshold=1.0)   # tracker.py:242
                if E is not None:
                    n_in, R, t, _ = geom.recover_pose(E, p1, p2, K, mask)                          # tracker.py:249
                    poses.append((R, t))
                    track_pose(R, t, frame, kps, desc, idx)
                    if idx % 5 == 0:
                        print("frame %d: %d matches, %d pose inliers, t = %s" % (idx, len(m), n_in, np.round(t.ravel(), 3)))
                    last = (kps, desc)
                    continue
            if args.relocalize:
                relocalize(frame, kps, desc, idx)
        last = (kps, desc)
    dt = time.perf_counter() - t0
    print("%d frames in %.2f s (%.1f frames/s through the Python drop-in classes), state %s, %d poses"
          % (n_seen, dt, n_seen / max(dt, 1e-9), state, len(poses)))
    if mapper is not None:
        mapper.save_map()
        print("map statistics: %s" % mapper.get_map_statistics())
        if args.merge_into:   # two sessions, one map: the saved mapper is the base, this run's map its tail
            base = LocalMapper.load_state(args.merge_into, context=mapper.ctx, output_path=args.map)
            if base.vocabulary is None:
                ensure_vocabulary(n_seen)   # (--vocabulary: loaded at the start, or trained on this run's keyframes now)
                if mapper.vocabulary is not None:
                    base.set_vocabulary(mapper.vocabulary)
            if base.vocabulary is None:
                print("--merge-into: neither %s nor this run carries a vocabulary; the maps are not merged" % args.merge_into)
            else:
                res = base.merge_map(mapper)
                print("merged into %s: aligned %s after %d tries%s; %d keyframes, %d map points"
                      % (args.merge_into, res["aligned"], res["tries"],
                         ", keyframe %d onto %d at scale %.4f, %d duplicates fused" % (res["kf_pos"], res["cand_pos"], res["scale"], res["correct"]["n_absorbed"])
                         if res["aligned"] else " (the run's map was taken out again)", len(base.keyframes), len(base.map_points)))
                mapper = base
                mapper.save_map()
        if args.save_state:
            mapper.save_state(args.save_state)
            print("state saved to %s (%d bytes)" % (args.save_state, os.path.getsize(args.save_state)))
        if args.local_ba:
            print("bundle adjustment: %d calls, %d ok" % (n_ba[0], n_ba[1]))
            if args.ba_covisible or args.ba_erase_outliers:
                print("bundle adjustment sets: %s, %d outlier observations erased, %d points left with fewer than two"
                      % ("covisible" if args.ba_covisible else "window", n_ba_erased[0], n_ba_erased[1]))
        if args.grow_neighbours:
            print("growth from neighbours: %d calls, %d points created with %d observations" % (n_grow[0], n_grow[1], n_grow[2]))
        if args.detect_loops:
            print("loop detection: %d calls, %d loops found" % (n_loop[0], n_loop[1]))
        if args.cull_points:
            a = mapper.arrays()
            print("point cull: %d frames noted, %d calls, %d points removed of %d tested; %d map points, %.2f observations per point"
                  % (tuple(n_ptcull) + (len(mapper.map_points), len(a["obs_kf"]) / max(len(mapper.map_points), 1))))
        if args.cull_keyframes:
            a = mapper.arrays()
            print("keyframe cull: %d calls, %d keyframes removed, %d kept; %d map points, %.2f observations per point"
                  % (n_cull[0], n_cull[1], len(mapper.keyframes), len(mapper.map_points), len(a["obs_kf"]) / max(len(mapper.map_points), 1)))
        if args.fuse:
            print("fusion: %d calls, %d points absorbed, %d observations gained" % (n_fuse[0], n_fuse[1], n_fuse[2]))
    return state, poses, n_map


def _print_selection(idx, initializer):
    """--init-model-selection: what the last initialize() decided"""
    sel = initializer.last_selection if initializer.model_selection else None
    if sel is not None:
        print("frame %d: model %s, RH %.3f, parallax %.2f deg, good %d (H candidates %s), %s" % (
            idx, {1: "H", 0: "F"}.get(sel["model"], "none"), sel["RH"], sel["parallax"], sel["n_good"], list(map(int, sel["n_good_h"])),
            "accepted" if sel["accepted"] else "refused"))


def localize_line(idx, ok, T, info):
    """the line --localize prints for a frame: ok, keyframe id, inliers and the pose's 12 numbers as they round-trip"""
    pose = "none" if T is None else " ".join("%.17g" % v for v in np.asarray(T)[:3, :].ravel())
    return "frame %d: localize %s, keyframe id %s, %d inliers, pose %s" % (idx, "ok" if ok else "failed", info["kf_id"], info["n_inliers"], pose)


def run_localize(args, K, D, orb, extractor, source, limit, skip, t0):
    """--load-state FILE --localize: every selected frame relocalised in the loaded map, one by one or - with --batch N - a chunk of N
    at a time through LocalMapper.relocalize_batch on FrameStream's extraction.  The map is read, never changed."""
    import vslam_amd as V
    from vslam_amd.mapper import LocalMapper
    mapper = LocalMapper.load_state(args.load_state, output_path=args.map or None)
    print("loaded %s: %d keyframes, %d map points%s" % (args.load_state, len(mapper.keyframes), len(mapper.map_points),
                                                      ", vocabulary of %d words" % len(mapper.vocabulary) if mapper.vocabulary is not None else ""))
    if args.vocabulary and os.path.exists(args.vocabulary):   # (else the vocabulary the state embeds, if it has one)
        mapper.set_vocabulary(V.Vocabulary.load(args.vocabulary, context=mapper.ctx))
        print("vocabulary: %d words from %s" % (len(mapper.vocabulary), args.vocabulary))
    pre = args.reloc_preselect if args.reloc_preselect > 0 and mapper.vocabulary is not None else None

    def selected():
        seen = 0
        for idx, frame in enumerate(source):
            if seen >= limit:
                return
            if skip and idx % (skip + 1) != 0:
                continue
            seen += 1
            yield geom.undistort_image(frame, K, D) if np.any(D) else frame
    n_seen = n_ok = 0
    if args.batch > 0:
        from vslam_amd.stream import FrameStream
        frames = selected()
        first = next(frames, None)
        if first is None:
            return "TRACKING", [], 0
        h, w = first.shape[:2]
        prm = V.orb_params(nfeatures=orb["n_features"], scale_factor=orb["scale_factor"], nlevels=orb["n_levels"], fast_threshold=orb["min_threshold"])
        fs = FrameStream(K, width=w, height=h, channels=3 if first.ndim == 3 else 1, chunk=args.batch, prm=prm,
                         detector=V.DETECT_GRID if args.grid else V.DETECT_ORB, copy=True)

        def chain():
            yield first
            yield from frames

        def flush(chunk):
            oks, Ts, infos = mapper.relocalize_batch([(r.keypoints, r.descriptors) for r in chunk], preselect=pre)
            for r, ok, T, info in zip(chunk, oks, Ts, infos):
                print(localize_line(r.index, ok, T, info))
            return int(oks.sum())
        try:
            chunk = []
            for r in fs.run(chain()):
                n_seen += 1
                chunk.append(r)
                if len(chunk) == args.batch:
                    n_ok += flush(chunk)
                    chunk = []
            if chunk:
                n_ok += flush(chunk)
        finally:
            fs.close()
    else:
        for idx, frame in enumerate(selected()):
            n_seen += 1
            if args.grid:
                kps, desc = extractor.distribute_keypoints(frame, aligned=True)
            else:
                kps, desc = extractor.extract_features(frame, distributed=False)
            ok, T, info = mapper.relocalize(kps, desc, preselect=pre)
            n_ok += bool(ok)
            print(localize_line(idx, ok, T, info))
    dt = time.perf_counter() - t0
    print("%d frames localised in %.2f s, %d ok%s%s" % (n_seen, dt, n_ok, ", chunks of %d" % args.batch if args.batch > 0 else "",
                                                      "" if pre is None else ", preselect %d" % pre))
    mapper.close()
    return "TRACKING", [], 0


def run_batched(args, cfg, K, D, orb, mt, initializer, source, limit, skip, t0):
    """--batch N: the frame loop above with the extraction and the tracking step of EVERY frame taken from FrameStream (one batched
    device call per N frames).  Initialisation (the first frame pair that yields a map) goes through MapInitializer on the streamed
    keypoints / descriptors, exactly as Tracker does (tracker.py:162,168-170)."""
    import vslam_amd as V
    from orbslam2.types import KeyPointSeq
    from vslam_amd.stream import FrameStream

    def selected():
        seen = 0
        for idx, frame in enumerate(source):
            if seen >= limit:
                return
            if skip and idx % (skip + 1) != 0:
                continue
            seen += 1
            yield geom.undistort_image(frame, K, D) if np.any(D) else frame
    stack = None
    if args.frames and not os.path.isdir(args.frames) and not np.any(D) and not skip:   # a frame stack on disk: handed over as slices
        data = np.load(args.frames)   # (read into memory: a memory-mapped stack would page-fault inside the staging copies)
        arr = data[sorted(data.files)[0]] if hasattr(data, "files") else data
        stack = np.ascontiguousarray(arr[:limit] if limit < 10 ** 9 else arr, dtype=np.uint8)
    frames = iter(stack) if stack is not None else selected()
    first = next(frames, None)
    if first is None:
        return "NOT_INITIALIZED", [], 0
    h, w = first.shape[:2]
    prm = V.orb_params(nfeatures=orb["n_features"], scale_factor=orb["scale_factor"], nlevels=orb["n_levels"], fast_threshold=orb["min_threshold"])
    fs = FrameStream(K, width=w, height=h, channels=3 if first.ndim == 3 else 1, chunk=args.batch, prm=prm,
                     detector=V.DETECT_GRID if args.grid else V.DETECT_ORB, ratio=mt["ratio_threshold"], disp_frac=0.02, thr_px=1.0, copy=False)
    # (copy=False: the results are views of the stream's pinned buffers, valid while iterating; what this loop keeps - the keypoints and
    #  descriptors the initialiser holds on to, the poses - is copied explicitly.  A tracking frame only reads its pose: 12 doubles.)
    matcher = DescriptorMatcher(mt["matcher_type"], ratio_threshold=mt["ratio_threshold"])
    kept = {0: first}   # (frames the initialiser may still want: the first one, and the one being initialised against)

    def chain():
        yield first
        for i, f in enumerate(frames, 1):
            if state[0] == "NOT_INITIALIZED":
                kept[i] = f
            yield f
    feed = stack if stack is not None else chain()
    frame_at = (lambda i: stack[i]) if stack is not None else (lambda i: kept.get(i, first))
    state, poses, n_map, n_seen = ["NOT_INITIALIZED"], [], 0, 0
    try:
        t_steady, n_steady = None, 0
        for r in fs.run(feed):
            n_seen += 1
            if n_seen == 3 * args.batch + 1:     # (steady state: context, plan and the three lanes warmed up by the first chunks)
                t_steady, n_steady = time.perf_counter(), n_seen - 1
            if state[0] == "NOT_INITIALIZED":
                kps, desc = KeyPointSeq(r.keypoints.copy()), r.descriptors.copy()
                if initializer.first_frame_keypoints is None:
                    initializer.set_first_frame(kps, desc, frame_at(r.index))
                else:
                    ok, R, t, pts, matches = initializer.initialize(kps, desc, matcher, frame_at(r.index))
                    _print_selection(r.index, initializer)
                    if ok:
                        state[0], n_map = "TRACKING", len(pts)
                        kept.clear()
                        poses.append((R, t))
                        print("frame %d: initialised, %d map points, t = %s" % (r.index, n_map, np.round(t.ravel(), 3)))
            else:
                p = r.pair
                if p is not None and p.ok:
                    poses.append((p.R.copy(), p.t.copy()))
                    if r.index % 100 == 0:
                        print("frame %d: %d pose inliers, t = %s" % (r.index, int(p.inlier.sum()), np.round(p.t.ravel(), 3)))
    finally:
        fs.close()
    t_end = time.perf_counter()
    dt = t_end - t0
    steady = "" if t_steady is None else "; %.0f frames/s from the fourth chunk on" % ((n_seen - n_steady) / max(t_end - t_steady, 1e-9))
    print("%d frames in %.2f s (%.1f frames/s through FrameStream incl. start-up, chunks of %d%s), state %s, %d poses"
          % (n_seen, dt, n_seen / max(dt, 1e-9), args.batch, steady, state[0], len(poses)))
    return state[0], poses, n_map


if __name__ == "__main__":
    main()
