"""Command line of the MI355X rain renderer.  It accepts the flag set of the reference's
main.py (main.py:15-127) and derives the same fields for Generator (main.py:131-161, particle
files main.py:187-220), so an existing invocation keeps working:

    python rain-rendering_amd/main.py --dataset kitti --intensity 25 --frame_end 10
    python -m torch.distributed.run --nproc-per-node 8 rain-rendering_amd/main.py --dataset kitti ...

Missing particle files are produced by this build's own generator (tools/particles.py) where the
reference would start its external, closed-source simulator."""
import argparse
import glob
import math
import os
import sys
import warnings

import numpy as np

if __package__ in (None, ''):
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _pkg = importlib.import_module('rain-rendering_amd')
    db = importlib.import_module('rain-rendering_amd.common.db')
    my_utils = importlib.import_module('rain-rendering_amd.common.my_utils')
    Generator = importlib.import_module('rain-rendering_amd.common.generator').Generator
else:
    from .common import db, my_utils
    from .common.generator import Generator

np.random.seed(0)
warnings.filterwarnings("ignore")

_J = os.path.join
# (flags, argparse keywords): names, types and defaults are the reference's; the wording is ours
_FLAGS = [
    (('--dataset',), dict(type=str, required=True, help='dataset name; its data lives in <dataset_root>/<dataset>')),
    (('-k', '--dataset_root'), dict(default=_J('data', 'source'), help='root of the source datasets')),
    (('-p', '--post_fix'), dict(type=str, default='', help='suffix of a GAN-translated dataset variant')),
    (('-s', '--sequences'), dict(default='', help='comma separated sequence prefixes to keep')),
    (('-ns', '--noise_scale'), dict(type=float, default=0.0, help='scale of the angular streak noise')),
    (('-nv', '--noise_std'), dict(type=float, default=0.0, help='standard deviation of the angular streak noise (degrees)')),
    (('-oa', '--opacity_attenuation'), dict(type=float, default=1.0, help='rain layer opacity factor in [0, 1]')),
    (('-r', '--particles'), dict(default=_J('data', 'particles'), help='root of the particle simulations')),
    (('-sd', '--streaks_db'), dict(default=_J('3rdparty', 'rainstreakdb'), help='Garg & Nayar rain streak database')),
    (('-i', '--intensity'), dict(type=str, default='25', help='fall rates in mm/hr, comma separated (e.g. 1,15,25,50)')),
    (('-d', '--depth'), dict(default=_J('data', 'source'), help='root of the depth maps')),
    (('-fs', '--frame_start'), dict(type=int, default=0, help='first frame index')),
    (('-fe', '--frame_end'), dict(type=int, default=None, help='one past the last frame index')),
    (('-fst', '--frame_step'), dict(type=int, default=1, help='frame stride')),
    (('-ff', '--frames'), dict(type=str, default='', help='explicit comma separated frame indices')),
    (('--conflict_strategy',), dict(type=str, default='overwrite', choices=['overwrite', 'skip', 'rename_folder'],
                                    help='what to do when the output folder exists')),
    (('--rendering_strategy',), dict(type=str, default=None, choices=[None, 'white', 'naive_db'], help="None (photometric) or 'white'")),
    (('--output',), dict(default=_J('data', 'output'), help='output root')),
    (('--save_envmap',), dict(action='store_true', help='also write the estimated environment maps')),
    (('--noverbose',), dict(action='store_true', help='no progress output')),
    (('--force_particles',), dict(action='store_true', help='(reference only) re-run the particle simulator')),
    (('--device_particles',), dict(action='store_true', help='simulate the rain particles on the GPU, frame by frame (no particle '
                                                             'file is read or written; this build only)')),
    (('--particle_model',), dict(type=str, default='iid', choices=['iid', 'field', 'rig'],
                                 help="with --device_particles: 'iid' draws independent particles for every simulated frame; 'field' is "
                                      "a persistent particle field for video: frame k + 1 shows the drops of frame k a little lower and "
                                      "closer (not with --noise_std); 'rig' is that field seen by one camera of a rig (--rig, --rig_view)")),
    (('--particle_draws',), dict(type=str, default='stream', choices=['stream', 'counter'],
                                 help="with --device_particles: 'stream' picks every drop's texture from numpy's stream seeded per frame, "
                                      "like the reference; 'counter' takes the pick from the drop's own random counter: a drop keeps its "
                                      "texture over its life (--particle_model field) and across the views of a rig, and the GPU skips its "
                                      "one serial pass (not with --noise_std)")),
    (('--streak_jitter',), dict(type=float, default=0.0,
                                help="with --device_particles: turn every streak by DEG degrees times a standard normal deviate of the "
                                     "drop's own (from its random counter: a drop keeps its tilt over its life and across the views of a "
                                     "rig); any --particle_model and --particle_draws; 0: off (not with --noise_std)")),
    (('--wind',), dict(type=str, default=None,
                       help="with --device_particles: WX,WZ, the air's mean horizontal velocity in m/s (x right, z toward the viewer; the "
                            "rig's axes under --particle_model rig, the world's under --trajectory): 5,0 makes the rain fall at 40 degrees to "
                            "the vertical, small drops leaning more than large ones; any --particle_model, --particle_draws and "
                            "--streak_jitter")),
    (('--gusts',), dict(type=str, default=None,
                        help="with --device_particles --particle_model field|rig: SIGMA[,TAU[,SEED]], a wind that changes over time on top "
                             "of --wind: per component an Ornstein-Uhlenbeck velocity of standard deviation SIGMA m/s (0 < SIGMA <= 20) and "
                             "correlation time TAU seconds (default 2), from SEED (default 0), over the run's frame indices: the slant "
                             "sways over seconds, coherently for every drop and every view")),
    (('--showers',), dict(type=str, default=None,
                          help="with --device_particles --particle_model field|rig: LOW,PERIOD_S[,PHASE], a rain rate that changes over "
                               "time: it swings between LOW mm/hr (0 <= LOW <= --intensity) and the run's --intensity, its peak, once every "
                               "PERIOD_S seconds (PHASE radians, default 0: the run starts at LOW), over the run's frame indices.  One rain "
                               "field builds, peaks and fades: drops that fall keep falling, each frame's fog follows its own rate; works "
                               "with --wind, --gusts, --trajectory, --rig, both --particle_draws and --streak_jitter")),
    (('--streak_lean',), dict(type=str, default='auto', choices=['auto', 'on', 'off'],
                              help="'on': a streak tile's lean and corner come from the streak's own end points; 'off': the reference's rule "
                                   "(lean by the image half the streak ends in, corner at its start: right for streaks that radiate from the "
                                   "image centre); 'auto' (default): on exactly when a non-zero --wind or --gusts is given")),
    (('--rig',), dict(type=str, default=None, help="with --particle_model rig: 'mono' (one camera), 'stereo:<baseline in metres>' (KITTI: stereo:0.54; view 0 "
                                                   "left, view 1 right) or a JSON file {\"views\": [{\"R\": [...9], \"c\": [...3]}, ...]}")),
    (('--trajectory',), dict(type=str, default=None,
                             help="with --device_particles --particle_model rig (a single camera: --rig mono): a poses file, 12 numbers per "
                                  "line (the 3 x 4 camera-to-world matrix, row by row, as KITTI odometry's poses.txt); row f is the pose of "
                                  "rendered frame f: the rain field is seen from a camera that moves and turns along it")),
    (('--trajectory_convention',), dict(type=str, default='kitti', choices=['kitti', 'native'],
                                        help="axes of --trajectory: 'kitti' (x right, y down, z forward) or 'native' (x right, y up, "
                                             "looking along -z)")),
    (('--lens_drops',), dict(type=str, default=None,
                             help="drops on the lens (the windshield): COUNT[,SEED] adherent raindrops (at most 128) that sit still for "
                                  "seconds and are then replaced elsewhere, or a JSON file of tools/lens.py LensDrops keywords (count, radius, "
                                  "aspect, mag, blur, edge, rim, life_s, hz, seed); frame i of a sequence wears the drops of time i / the "
                                  "dataset's frame rate; with and without --device_particles, any --particle_model (rig: the drops of "
                                  "--rig_view's own lens).  The rain mask does not show them")),
    (('--lens_alpha',), dict(action='store_true', help="with --lens_drops: also write <out_dir>/lens_alpha/<name>.png, the per-pixel "
                                                       "coverage of the drops on the lens as a grey level (0: no drop, 255: all drop)")),
    (('--rain_layer',), dict(action='store_true', help="also write <out_dir>/rain_layer/<name>.png: the frame's streaks alone as a "
                                                       "straight-alpha RGBA PNG (colour L over transparency, alpha 1 - T; any viewer shows "
                                                       "it), the frame's mean shift in its tEXt chunk `rain-shift`; "
                                                       "common.imgops.read_rain_layer reads it back.  rainy = T x fogged background + L - shift")),
    (('--device_resize',), dict(action='store_true',
                               help="resize full-size frames on the GPU: where a dataset renders at a fraction of its files' resolution "
                                    "(render_scale / depth_scale other than 1) the batch-native route uploads the files' own scanlines and the "
                                    "library resizes image and depth map on the device (rr_set_input_resize) instead of on the host; the "
                                    "output files are the same, byte for byte.  Without a resize to do the flag changes nothing.  JPEG frames at "
                                    "such a scale stay on the host-resize path: their device decode (IDCT and colour) runs at render scale 1 only.  "
                                    "(At render scale 1 a tree of baseline .jpg / .jpeg frames is decoded that way by itself; a frame of such a tree "
                                    "that the JPEG reader refuses -- progressive, damaged, another size or chroma sampling -- is SKIPPED with a "
                                    "message: no output files are written for it)")),
    (('--rig_view',), dict(type=int, default=0, help="with --particle_model rig: the view this run's camera folder shows; one run per "
                                                     "camera folder with the same seed gives a coherent set")),
]


def _parse(argv):
    ap = argparse.ArgumentParser(description='Rain rendering on MI355X (hot path in librainhip.so)')
    for names, kw in _FLAGS:
        ap.add_argument(*names, **kw)
    return ap.parse_args(argv)


def _wind_and_lean(ns):
    """--wind WX,WZ as a pair of floats (default (0, 0)), --gusts SIGMA[,TAU[,SEED]] as (sigma, tau, seed) or None, --showers
    LOW,PERIOD_S[,PHASE] as (low, period_s, phase) or None, and --streak_lean as ns.lean: 'auto' is on exactly when a non-zero wind or
    a gust series is given, so that no command line without --wind or --gusts changes its output."""
    wind = getattr(ns, 'wind', None)
    if wind is not None and not isinstance(wind, tuple):
        try:
            wind = tuple(float(v) for v in str(wind).split(','))
        except ValueError:
            wind = ()
        if len(wind) != 2 or not all(math.isfinite(v) and abs(v) <= 100.0 for v in wind):
            raise SystemExit("--wind %r: expected WX,WZ, two finite numbers of m/s of magnitude <= 100" % (ns.wind,))
        if any(wind) and not ns.device_particles:
            raise SystemExit("--wind needs --device_particles (the wind moves the particles the GPU's generator makes)")
    ns.wind = wind if wind is not None else (0.0, 0.0)
    gusts = getattr(ns, 'gusts', None)
    if gusts is not None and not isinstance(gusts, tuple):     # --gusts SIGMA[,TAU[,SEED]] as (sigma, tau, seed)
        parts = str(gusts).split(',')
        try:
            gusts = (float(parts[0]), float(parts[1]) if len(parts) > 1 else 2.0, int(parts[2]) if len(parts) > 2 else 0)
        except ValueError:
            gusts = ()
        if not 1 <= len(parts) <= 3 or len(gusts) != 3 or not (math.isfinite(gusts[0]) and 0 < gusts[0] <= 20.0) or \
                not (math.isfinite(gusts[1]) and gusts[1] > 0) or not 0 <= gusts[2] < 2 ** 32:
            raise SystemExit("--gusts %r: expected SIGMA[,TAU[,SEED]] with 0 < SIGMA <= 20 m/s, TAU > 0 seconds, SEED an integer in "
                             "[0, 2^32)" % (ns.gusts,))
        if not ns.device_particles or getattr(ns, 'particle_model', 'iid') not in ('field', 'rig'):
            raise SystemExit("--gusts needs --device_particles --particle_model field|rig (the i.i.d. model has no time)")
    ns.gusts = gusts
    showers = getattr(ns, 'showers', None)
    if showers is not None and not isinstance(showers, tuple):  # --showers LOW,PERIOD_S[,PHASE] as (low, period_s, phase)
        parts = str(showers).split(',')
        try:
            showers = (float(parts[0]), float(parts[1]), float(parts[2]) if len(parts) > 2 else 0.0)
        except (ValueError, IndexError):
            showers = ()
        try:                                                    # the peak is the run's --intensity: every one of them
            peaks = [float(v) for v in (ns.intensity.split(',') if isinstance(ns.intensity, str) else ns.intensity)]
        except (ValueError, TypeError, AttributeError):
            peaks = []
        if not 2 <= len(parts) <= 3 or len(showers) != 3 or not (math.isfinite(showers[0]) and showers[0] >= 0) or \
                not (math.isfinite(showers[1]) and showers[1] > 0) or not math.isfinite(showers[2]) or any(showers[0] > p for p in peaks):
            raise SystemExit("--showers %r: expected LOW,PERIOD_S[,PHASE] with 0 <= LOW <= --intensity mm/hr, PERIOD_S > 0 seconds, PHASE a "
                             "finite number of radians" % (ns.showers,))
        if not ns.device_particles or getattr(ns, 'particle_model', 'iid') not in ('field', 'rig'):
            raise SystemExit("--showers needs --device_particles --particle_model field|rig (the i.i.d. model has no time)")
    ns.showers = showers
    mode = getattr(ns, 'streak_lean', 'auto') or 'auto'
    ns.lean = (any(ns.wind) or ns.gusts is not None) if mode == 'auto' else mode == 'on'
    return ns


def _lens(ns):
    """--lens_drops SPEC is checked here as far as it can be without the frame size (the Generator builds the LensDrops at the rendered
    size): a trial instance at 64 x 64 and 10 Hz refuses what every size refuses.  --lens_alpha needs it."""
    spec = getattr(ns, 'lens_drops', None)
    if getattr(ns, 'lens_alpha', False) and spec is None:
        raise SystemExit("--lens_alpha needs --lens_drops (the label file shows the drops on the lens)")
    if spec is not None and not isinstance(spec, str):
        raise SystemExit("--lens_drops %r: expected COUNT[,SEED] or the path of a JSON file" % (spec,))
    if spec is not None:
        if __package__ in (None, ''):
            lens = importlib.import_module('rain-rendering_amd.tools.lens')
        else:
            from .tools import lens
        try:
            lens.LensDrops.from_spec(spec, 64, 64, 10.0)
        except ValueError as e:
            raise SystemExit("--lens_drops %r: %s" % (spec, e))
    return ns


def _derive(ns):
    """The fields the reference computes after parsing (main.py:131-161)."""
    if ns.force_particles and ns.conflict_strategy == "skip":
        raise AssertionError("If particles simulator is forced, cannot skip")
    if getattr(ns, 'particle_model', 'iid') != 'iid':
        if not ns.device_particles:
            raise SystemExit("--particle_model %s needs --device_particles (the particle files hold the i.i.d. model)" % ns.particle_model)
        if ns.noise_std:
            raise SystemExit("--noise_std cannot be combined with --particle_model field: the reference's angular noise turns a shared "
                             "simulated frame in place and has no meaning for particles that move from frame to frame")
    if (getattr(ns, 'particle_model', 'iid') == 'rig') != (getattr(ns, 'rig', None) is not None):
        raise SystemExit("--particle_model rig and --rig go together")
    if getattr(ns, 'trajectory', None) is not None and (getattr(ns, 'particle_model', 'iid') != 'rig' or not ns.device_particles):
        raise SystemExit("--trajectory needs --device_particles --particle_model rig (a single camera: --rig mono)")
    if getattr(ns, 'particle_draws', 'stream') != 'stream':
        if not ns.device_particles:
            raise SystemExit("--particle_draws %s needs --device_particles (a particle file's frames are drawn from numpy's stream)" %
                             ns.particle_draws)
        if ns.noise_std:
            raise SystemExit("--noise_std cannot be combined with --particle_draws counter: the angular noise needs the stream's normal "
                             "deviates and the order of the run")
    jitter = getattr(ns, 'streak_jitter', 0.0) or 0.0
    if not math.isfinite(jitter) or jitter < 0:
        raise SystemExit("--streak_jitter %r: expected a finite number of degrees >= 0" % (jitter,))
    if jitter:
        if not ns.device_particles:
            raise SystemExit("--streak_jitter needs --device_particles (the jitter is made by the GPU's particle generator)")
        if ns.noise_std:
            raise SystemExit("--streak_jitter cannot be combined with --noise_std: the jitter is a function of the drop, the angular "
                             "noise of the order of the run")
    _wind_and_lean(ns)
    _lens(ns)
    ns.verbose = not ns.noverbose
    light_db = _J(ns.streaks_db, 'env_light_database')
    ns.texture = _J(light_db, 'size32')
    ns.norm_coeff = _J(light_db, 'txt', 'normalized_env_max.txt')
    for what, path in (("rainstreakdb database is missing.", ns.streaks_db),
                       ("rainstreakdb database is not valid. Some files are missing.", ns.texture),
                       ("rainstreakdb database is not valid. Some files are missing.", ns.norm_coeff)):
        assert os.path.exists(path), (what, path)
    ns.intensity = [int(v) for v in ns.intensity.split(",")]
    ns.frames = [int(v) for v in ns.frames.split(",")] if ns.frames else ns.frames
    base_name = ns.dataset[:-4] if "_gan" in ns.dataset else ns.dataset
    ns.dataset_root = _J(ns.dataset_root, base_name)
    ns.depth_root = _J(ns.depth, base_name)
    ns.images_root = ns.dataset_root
    ns.calib = None
    assert os.path.exists(ns.images_root), ("Dataset folder does not exist.", ns.images_root)
    wanted = ns.sequences.split(',')
    ns = db.resolve_paths(ns.dataset, ns)                   # dataset plug-in: fills sequences / images / depth / calib
    ns.settings = db.settings(ns.dataset)
    ns.sequences = np.asarray([s for s in ns.sequences if any(s.startswith(w) for w in wanted)])
    ns.weather = np.asarray([dict(weather="rain", fallrate=r) for r in ns.intensity])
    return ns


def _exists(entry):
    if entry is None:
        return True
    return all(os.path.exists(e) for e in entry) if isinstance(entry, list) else os.path.exists(entry)


def _drop_incomplete_sequences(ns):
    """A sequence needs its image folder, depth folder and (if the plug-in names one) calibration."""
    print("\nChecking sequences...")
    print(" {} sequences found: {}".format(len(ns.sequences), list(ns.sequences)))
    for seq in list(ns.sequences):
        problems = [(kind, tree[seq]) for kind, tree in (("images folder", ns.images), ("depth folder", ns.depth),
                                                         ("calib data", ns.calib)) if not _exists(tree[seq])]
        for kind, where in problems:
            print(" Skip sequence '{}': {} is missing {}".format(seq, kind, where))
        if problems:
            ns.sequences = ns.sequences[ns.sequences != seq]
            for tree in (ns.images, ns.depth, ns.calib):
                del tree[seq]
    print("Found {} valid sequence(s): {}".format(len(ns.sequences), list(ns.sequences)))


def _locate_particles(ns):
    """One particle file per (sequence, fall rate) (reference main.py:187-220).  Where the reference launches the external
    weather-particle-simulator for missing (or --force_particles) files, this build runs its own generator
    (tools/particles.py: same settings in, same XML schema out; there is no source of the reference's simulator).

    Under several ranks (torch.distributed.run) rank 0 alone looks, generates and decides; the others receive its list
    (sharding.rank0_decides: a broadcast, which also holds them back until the files are complete).  Every rank
    regenerating the same file, or globbing while a peer rewrites it, would hand the loader a half-written file."""
    if __package__ in (None, ''):
        particles = importlib.import_module('rain-rendering_amd.tools.particles')
        sharding = importlib.import_module('rain-rendering_amd.sharding')
    else:
        from .tools import particles
        from . import sharding
    root = _J(ns.particles, ns.dataset)
    if getattr(ns, 'device_particles', False):
        # BASELINE.json configs[4] from the command line: no XML at all -- the generator's settings go to the GPU with every
        # batch (rr_frame_in.sim) and the drop tables are born there (same model, seed 0, as the files simulate() writes)
        ns.sim_options = {seq: db.sim(ns.dataset, seq, root)["options"] for seq in ns.sequences}
        ns.particles = {seq: [None] * len(ns.weather) for seq in ns.sequences}
        return

    def locate():
        print("\nResolving particles simulations...")
        found = {}
        n_run = 0
        for seq in ns.sequences:
            sim = db.sim(ns.dataset, seq, root)
            found[seq] = []
            for w in ns.weather:
                have = sorted(glob.glob(my_utils.particles_path(sim["path"], w)))
                if ns.force_particles or not have:
                    if n_run == 0:
                        print(" particles simulations to compute...")
                    n_run += 1
                    path = particles.simulate(sim, w, force_recompute=True)      # the file just written, not a re-glob:
                    print("  " + path)                                           # a stale *_camera0.xml may sit beside it
                    found[seq].append(path)
                else:
                    found[seq].append(have[0])
        print(" All particles simulations ready" if n_run == 0 else " All particles simulation completed")
        return found
    ns.particles = sharding.rank0_decides(locate, *sharding.rank_world())


def check_arg(argv):
    ns = _derive(_parse(argv))
    _drop_incomplete_sequences(ns)
    _locate_particles(ns)
    return ns


def main(argv=None):
    print("\nBuilding internal parameters...")
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:      # before anything rank 0 decides for the others (particle files)
        import torch
        import torch.distributed as dist
        # RAIN_DEVICE pins every rank to one device and RAIN_DIST_BACKEND=gloo replaces RCCL (which refuses two ranks on one
        # GPU): how the GPU test tier runs this driver under N > 1 on the one GPU it has (tests/test_gpu_driver.py)
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get('RAIN_DEVICE', os.environ.get('LOCAL_RANK', '0'))))
        if not dist.is_initialized():
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            dist.init_process_group(os.environ.get('RAIN_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo'))
    args = check_arg(sys.argv[1:] if argv is None else argv)
    print("\nRunning renderers...")
    generator = Generator(args)
    generator.run()
    return generator


if __name__ == "__main__":
    main()
