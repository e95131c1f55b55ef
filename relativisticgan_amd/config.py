"""The reference's command-line surface (GLI:14-62): same flag names, types, defaults.

Plus this build's own switches (prefixed ``--rgan_``), which the reference lacks:
``--rgan_rng`` (``host``: draw z/u/batches from the CPU generators in the reference's
order, bit-compatible inputs; ``device``: draw on the GPU, for throughput runs) and
``--rgan_sync_bn`` (BatchNorm statistics under data parallelism: default off = the
reference's DataParallel, each rank normalises with its own shard; on = SyncBN over the
global batch), ``--rgan_diffaug`` (differentiable augmentation of D's inputs, off by
default; relativisticgan_amd/augment.py; its strength: ``--rgan_aug_p P``, each transform applied
to a sample with probability P, and ``--rgan_ada_target T`` with ``--rgan_ada_interval`` /
``--rgan_ada_kimg``, P adapted during training, see ``validate_ada``), ``--rgan_ema_G BETA`` with ``--rgan_ema_warmup``
(an exponential moving average of G's weights, kept next to G, checkpointed, sampled and used
for the extra images; 0 = off, the default; relativisticgan_amd/ema.py), ``--rgan_r1 GAMMA`` /
``--rgan_r2 GAMMA`` with ``--rgan_reg_every K`` (the zero-centred gradient penalties
GAMMA / 2 * mean ||dD/dx||^2 on the real / on the generated batch D saw, added to the D step
after errD and the WGAN-GP penalty; lazily every K-th iteration with weight GAMMA * K, see
``reg_weight``; 0 = off, the default; not with --rgan_pac 2), ``--rgan_lecam LAMBDA``
with ``--rgan_lecam_beta`` / ``--rgan_lecam_start`` (LeCam regularisation: LAMBDA times the squared
distance of D's outputs from moving averages of its outputs on the other kind of batch, added to
the D step without another pass of D; 0 = off, the default; see ``validate_lecam``),
``--rgan_swd_every K`` with ``--rgan_swd_images N`` (log the sliced Wasserstein distance between
the training images and G's samples after every K-th iteration; 0 = off, the default;
single-process runs only, see ``validate_swd``; relativisticgan_amd/swd.py), ``--rgan_nn_every K`` /
``--rgan_nn True`` with ``--rgan_nn_images``, ``--rgan_nn_side`` and ``--rgan_nn_k`` (each generated
image's nearest training images as a grid, and k-NN precision / recall in pixel space, during
training / in evaluate; off by default; see ``validate_nn``; relativisticgan_amd/neighbours.py), ``--rgan_pac 2``
(the PacGAN-2 script, code/GAN_losses_iter_PAC.py, which shares this CLI) and
``--rgan_script`` (the defaults of GAN_losses_iter / GAN_losses_iter_art / GAN_losses_iter_PAC).
"""
import argparse


def str_to_bool(s):
    """GLI:14-15."""
    return s.lower() in ("true", "yes", "on", "t", "1")


_FLAGS = [
    ("image_size", int, 64), ("batch_size", int, 32), ("n_colors", int, 3), ("z_size", int, 128),
    ("G_h_size", int, 128), ("D_h_size", int, 128), ("lr_D", float, .0001), ("lr_G", float, .0001),
    ("n_iter", int, 100000), ("beta1", float, 0.5), ("beta2", float, 0.999), ("decay", float, 0),
    ("SELU", "bool", False), ("NN_conv", "bool", False), ("seed", int, None),
    ("input_folder", str, "/home/alexia/Datasets/Meow_64x64"),
    ("output_folder", str, "/home/alexia/Dropbox/Ubuntu_ML/Output/GANlosses"),
    ("inception_folder", str, "/home/alexia/Inception"), ("load", str, None), ("cuda", "bool", True),
    ("n_gpu", int, 1), ("loss_D", int, 1), ("Diters", int, 1), ("Giters", int, 1), ("penalty", float, 10),
    ("spectral", "bool", False), ("spectral_G", "bool", False), ("weight_decay", float, 0),
    ("gen_extra_images", int, 50000), ("gen_every", int, 100000), ("extra_folder", str, "/home/alexia/Output/Extra"),
    ("show_graph", "bool", False), ("no_batch_norm_G", "bool", False), ("no_batch_norm_D", "bool", False),
    ("Tanh_GD", "bool", False), ("grad_penalty", "bool", False), ("arch", int, 0), ("print_every", int, 1000),
    ("save", "bool", True), ("CIFAR10", "bool", False), ("CIFAR10_input_folder", str, "/home/alexia/Datasets/CIFAR10"),
]


# code/GAN_losses_iter_art.py is GLI with these defaults (its only differences, art:20-60)
ART_DEFAULTS = {
    "image_size": 128, "loss_D": 7, "gen_extra_images": 2000, "gen_every": 2000,
    "input_folder": "/home/ubuntu/datasets/meow_128x128", "output_folder": "/home/ubuntu/RelativisticGAN/output",
    "inception_folder": "/home/ubuntu/models/Inception", "extra_folder": "/home/ubuntu/RelativisticGAN/extra",
    "CIFAR10_input_folder": "/home/ubuntu/datasets/CIFAR10",
}
SCRIPTS = ("GAN_losses_iter", "GAN_losses_iter_art", "GAN_losses_iter_PAC")


LECAM_DEFAULTS = (0.99, 1)  # --rgan_lecam_beta, --rgan_lecam_start
NN_DEFAULTS = (8192, 64, 3)  # --rgan_nn_images, --rgan_nn_side, --rgan_nn_k
NN_SIDES = (8, 16, 32, 64)


def make_parser(script="GAN_losses_iter"):
    """The CLI of one of the reference's three training scripts (same flags; the art script
    changes defaults, the PAC script packs 2 samples for D)."""
    p = argparse.ArgumentParser(description="RelativisticGAN training (MI355X build)")
    p.register("type", "bool", str_to_bool)
    for name, typ, default in _FLAGS:
        if script == "GAN_losses_iter_art":
            default = ART_DEFAULTS.get(name, default)
        if typ is str:
            p.add_argument("--" + name, default=default)
        else:
            p.add_argument("--" + name, type=typ, default=default)
    p.add_argument("--rgan_script", choices=SCRIPTS, default=script,
                   help="which reference script's defaults/behaviour to follow")
    p.add_argument("--rgan_rng", choices=("host", "device"), default="host")
    p.add_argument("--rgan_sync_bn", type="bool", default=False)
    p.add_argument("--rgan_batch_D", type="bool", default=None,
                   help="run the D step's D(x) and D(x_fake) as one batched pass (per-call BN kept); "
                        "default: on (one process and data parallel)")
    p.add_argument("--rgan_batch_G", type="bool", default=None,
                   help="run the G step's D(G(z)) and D(x) (heads 5-8) as one batched pass (per-call BN "
                        "kept, gradient through the D(G(z)) half only); default: on")
    p.add_argument("--rgan_pac", dest="pac", type=int, default=2 if script == "GAN_losses_iter_PAC" else 1,
                   choices=(1, 2),
                   help="2 = PacGAN-2, the reference's code/GAN_losses_iter_PAC.py (D sees 2 samples packed "
                        "channel-wise)")
    p.add_argument("--rgan_diffaug", default="",
                   help="differentiable augmentation of every image D sees, reals and fakes, with G's gradient "
                        "flowing back through it: a comma-separated subset of color,translation,cutout,"
                        "xflip,rot90,warp (default '': off; not with --rgan_pac 2; the geometric xflip, rot90 "
                        "and warp leak into G when always on: give them --rgan_aug_p <= 0.8 or "
                        "--rgan_ada_target)")
    p.add_argument("--rgan_aug_p", type=float, default=None,
                   help="apply each --rgan_diffaug transform to a sample with this probability, in [0, 1]: the "
                        "fixed value, or with --rgan_ada_target the initial one (default unset: 1 without "
                        "adaptation, i.e. every transform on every image; 0 with it)")
    p.add_argument("--rgan_ada_target", type=float, default=0.0,
                   help="adapt the augmentation probability during training: raise it while r = mean sign(D(x_i) "
                        "- D(G(z_i))) over the (real, fake) pairs of D's steps exceeds T, lower it while r is "
                        "below; in (0, 1), e.g. 0.6 (default 0: no adaptation)")
    p.add_argument("--rgan_ada_interval", type=int, default=4,
                   help="adjust the probability after every K-th D step (default 4)")
    p.add_argument("--rgan_ada_kimg", type=float, default=500.0,
                   help="thousands of images over which the probability may cross from 0 to 1 (default 500)")
    p.add_argument("--rgan_ema_G", type=float, default=0.0,
                   help="keep an exponential moving average of G's weights with this decay, in [0, 1) (e.g. "
                        "0.999): checkpointed as G_ema, sampled next to G's own sample grid and used for the "
                        "extra images (default 0: off)")
    p.add_argument("--rgan_ema_warmup", type="bool", default=True,
                   help="ramp the moving average's decay as min(beta, (1 + t) / (10 + t)) over its first updates")
    p.add_argument("--rgan_r1", type=float, default=0.0,
                   help="zero-centred gradient penalty on the real batch D saw, R1 = GAMMA / 2 * mean "
                        "||dD(x)/dx||^2, added to the D step (default 0: off; not with --rgan_pac 2)")
    p.add_argument("--rgan_r2", type=float, default=0.0,
                   help="the same penalty on the (detached) generated batch D saw, R2 (default 0: off)")
    p.add_argument("--rgan_reg_every", type=int, default=1,
                   help="lazy regularisation: run R1 / R2 in every K-th iteration only (i %% K == 0), with "
                        "weight GAMMA * K (default 1: every iteration)")
    p.add_argument("--rgan_lecam", type=float, default=0.0,
                   help="LeCam regularisation of D (Tseng et al., CVPR 2021): add LAMBDA * (mean (D(x) - a_fake)^2 "
                        "+ mean (D(x_fake) - a_real)^2) to the D step, a_real / a_fake being moving averages of "
                        "D's outputs on the real / generated batches; meant to go with --rgan_diffaug; e.g. 0.3, "
                        "the paper's CIFAR value (default 0: off)")
    p.add_argument("--rgan_lecam_beta", type=float, default=LECAM_DEFAULTS[0],
                   help="decay of the LeCam anchors' moving averages, in [0, 1) (default 0.99)")
    p.add_argument("--rgan_lecam_start", type=int, default=LECAM_DEFAULTS[1],
                   help="the D-step count from which the LeCam term has weight (the anchors move from the first "
                        "step on); >= 1 (default 1)")
    p.add_argument("--rgan_perf_log", type="bool", default=True,
                   help="after each reference log line, a line with img/s and MFMA%% of the training "
                        "iterations since the previous one (sample PNGs, checkpoints and extra images excluded)")
    p.add_argument("--rgan_swd_every", type=int, default=0,
                   help="after every K-th iteration, log the sliced Wasserstein distance (x 1000, per Laplacian-"
                        "pyramid level and their average; Karras et al., ICLR 2018) between the training images and "
                        "G's samples (the averaged generator's with --rgan_ema_G); single-process runs only "
                        "(default 0: off)")
    p.add_argument("--rgan_swd_images", type=int, default=8192,
                   help="images per set for the sliced Wasserstein distance (--rgan_swd_every and "
                        "python -m relativisticgan_amd.evaluate), at most the dataset's size (default 8192)")
    p.add_argument("--rgan_nn_every", type=int, default=0,
                   help="after every K-th iteration, log the nearest-training-image line (median RMS pixel "
                        "difference of G's samples to their nearest training image, the same among the training "
                        "images, their ratio, and k-NN precision / recall; Kynkaanniemi et al., NeurIPS 2019, in "
                        "pixel space) and write images/nn_iterNNNNN.png, 8 samples next to their nearest training "
                        "images; single-process runs only (default 0: off)")
    p.add_argument("--rgan_nn", type="bool", default=False,
                   help="python -m relativisticgan_amd.evaluate: also print that line and write nn.png into "
                        "--output_folder (default False)")
    p.add_argument("--rgan_nn_images", type=int, default=NN_DEFAULTS[0],
                   help="training and generated images compared by --rgan_nn_every / --rgan_nn, at most the "
                        "dataset's size (default 8192)")
    p.add_argument("--rgan_nn_side", type=int, default=NN_DEFAULTS[1],
                   help="side to which images are box-averaged before they are compared: 8, 16, 32 or 64, a "
                        "divisor of --image_size (default 64)")
    p.add_argument("--rgan_nn_k", type=int, default=NN_DEFAULTS[2],
                   help="neighbours per image, 1..8: the grid's columns and the k of precision / recall (default 3)")
    p.add_argument("--rgan_synthetic", type=int, default=0,
                   help="use N synthetic images instead of an image folder (no torchvision here)")
    return p


def parse(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--rgan_script", choices=SCRIPTS, default="GAN_losses_iter")
    script = pre.parse_known_args(argv)[0].rgan_script
    parser = make_parser(script)
    ns = parser.parse_args(argv)
    try:
        from .augment import validate
        validate(ns.rgan_diffaug, ns.pac)
    except ValueError as e:
        parser.error(str(e))  # exits with the message
    if not 0.0 <= ns.rgan_ema_G < 1.0:
        parser.error(f"--rgan_ema_G must lie in [0, 1) (0 = off), got {ns.rgan_ema_G}")
    try:
        validate_reg(ns.rgan_r1, ns.rgan_r2, ns.rgan_reg_every, ns.pac)
        validate_ada(ns.rgan_diffaug, ns.rgan_aug_p, ns.rgan_ada_target, ns.rgan_ada_interval, ns.rgan_ada_kimg)
        validate_lecam(ns.rgan_lecam, ns.rgan_lecam_beta, ns.rgan_lecam_start)
        validate_swd(ns.rgan_swd_every, ns.rgan_swd_images, ns.image_size)
        validate_nn(ns.rgan_nn_every, ns.rgan_nn, ns.rgan_nn_images, ns.rgan_nn_side, ns.rgan_nn_k, ns.image_size)
    except ValueError as e:
        parser.error(str(e))
    return ns


def validate_swd(every, images=8192, image_size=64, world=None):
    """Check --rgan_swd_every / --rgan_swd_images (ValueError otherwise); True when the metric is on.
    Refused under data parallelism (WORLD_SIZE > 1): the metric runs G on one rank, and a SyncBN
    forward there would wait for the others."""
    import os
    if every < 0:
        raise ValueError(f"--rgan_swd_every must be >= 0 (0 = off), got {every}")
    if images < 1:
        raise ValueError(f"--rgan_swd_images must be >= 1, got {images}")
    if every == 0:
        return False
    if image_size < 32 or image_size & (image_size - 1):
        raise ValueError(f"--rgan_swd_every needs an --image_size that is a power of two >= 32, got {image_size}")
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    if world > 1:
        raise ValueError("--rgan_swd_every is for single-process runs: under data parallelism evaluate a checkpoint "
                         "with python -m relativisticgan_amd.evaluate instead")
    return True


def validate_nn(every=0, on=False, images=NN_DEFAULTS[0], side=NN_DEFAULTS[1], k=NN_DEFAULTS[2], image_size=64,
                world=None):
    """Check --rgan_nn_every / --rgan_nn / --rgan_nn_images / --rgan_nn_side / --rgan_nn_k (ValueError
    otherwise); True when the check is on.  The working side is min(side, image_size).  Refused
    under data parallelism (WORLD_SIZE > 1) for the reason ``validate_swd`` gives."""
    import os
    if every < 0:
        raise ValueError(f"--rgan_nn_every must be >= 0 (0 = off), got {every}")
    if not 1 <= k <= 8:
        raise ValueError(f"--rgan_nn_k must lie in 1..8, got {k}")
    if images < k + 1:
        raise ValueError(f"--rgan_nn_images must be >= --rgan_nn_k + 1 = {k + 1}, got {images}")
    if side not in NN_SIDES:
        raise ValueError(f"--rgan_nn_side must be one of 8, 16, 32, 64, got {side}")
    if every == 0 and not on:
        return False
    s = min(side, image_size)
    if s not in NN_SIDES or image_size % s or image_size // s > 32:
        raise ValueError(f"--rgan_nn_side {side} needs an --image_size it divides by at most 32 (or a smaller one in "
                         f"8, 16, 32, 64), got {image_size}")
    world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
    if world > 1:
        raise ValueError("--rgan_nn_every / --rgan_nn are for single-process runs: under data parallelism evaluate a "
                         "checkpoint with python -m relativisticgan_amd.evaluate --rgan_nn True instead")
    return True


ADA_DEFAULTS = (4, 500.0)  # --rgan_ada_interval, --rgan_ada_kimg


def validate_ada(policy, aug_p=None, target=0.0, interval=4, kimg=500.0):
    """Check --rgan_aug_p / --rgan_ada_target / --rgan_ada_interval / --rgan_ada_kimg (ValueError
    otherwise).  Returns ``(gated, p0)``: whether the transforms are gated at all (unset flags:
    no, the ungated path as before) and the fixed or initial probability."""
    target = float(target or 0.0)
    given = aug_p is not None or target != 0.0 or (interval, float(kimg)) != ADA_DEFAULTS
    if given and not (policy or "").strip(" ,"):
        raise ValueError("--rgan_aug_p / --rgan_ada_target / --rgan_ada_interval / --rgan_ada_kimg set the strength "
                         "of --rgan_diffaug: name the transforms there")
    if aug_p is not None and not 0.0 <= aug_p <= 1.0:
        raise ValueError(f"--rgan_aug_p must lie in [0, 1], got {aug_p}")
    if target != 0.0 and not 0.0 < target < 1.0:
        raise ValueError(f"--rgan_ada_target must lie in (0, 1) (0 = no adaptation), got {target}")
    if interval < 1:
        raise ValueError(f"--rgan_ada_interval must be >= 1, got {interval}")
    if not kimg > 0:
        raise ValueError(f"--rgan_ada_kimg must be > 0, got {kimg}")
    gated = aug_p is not None or target != 0.0
    return gated, float(aug_p) if aug_p is not None else (0.0 if target != 0.0 else 1.0)


def validate_reg(r1, r2, every, pac=1):
    """Check --rgan_r1 / --rgan_r2 / --rgan_reg_every (ValueError otherwise)."""
    for name, gamma in (("--rgan_r1", r1), ("--rgan_r2", r2)):
        if not gamma >= 0.0:
            raise ValueError(f"{name} must be >= 0 (0 = off), got {gamma}")
    if every < 1:
        raise ValueError(f"--rgan_reg_every must be >= 1, got {every}")
    if every > 1 and r1 == 0 and r2 == 0:
        raise ValueError("--rgan_reg_every > 1 needs --rgan_r1 or --rgan_r2: it schedules those penalties only")
    if (r1 > 0 or r2 > 0) and pac != 1:
        raise ValueError("--rgan_r1 / --rgan_r2 are not available with --rgan_pac 2")


def validate_lecam(lam, beta=LECAM_DEFAULTS[0], start=LECAM_DEFAULTS[1]):
    """Check --rgan_lecam / --rgan_lecam_beta / --rgan_lecam_start (ValueError otherwise).
    Returns whether the term is on."""
    lam = 0.0 if lam is None else lam
    if not lam >= 0.0:
        raise ValueError(f"--rgan_lecam must be >= 0 (0 = off), got {lam}")
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"--rgan_lecam_beta must lie in [0, 1), got {beta}")
    if start != int(start) or start < 1:
        raise ValueError(f"--rgan_lecam_start must be an integer >= 1, got {start}")
    if lam == 0 and (float(beta), int(start)) != LECAM_DEFAULTS:
        raise ValueError("--rgan_lecam_beta / --rgan_lecam_start need --rgan_lecam: they shape that term only")
    return lam > 0


def reg_weight(i, every, gamma):
    """Lazy regularisation (--rgan_reg_every K): the weight of a zero-centred penalty in
    iteration ``i`` -- gamma * K when i % K == 0 (the penalty then runs in each of that
    iteration's D steps), else 0 (it does not run).  Stateless, so a resumed run continues the
    schedule from its iteration number."""
    return float(gamma) * every if gamma > 0 and i % every == 0 else 0.0


def make_param(**overrides):
    """Namespace with the reference defaults, then ``overrides``."""
    ns = make_parser().parse_args([])
    for k, v in overrides.items():
        cur = getattr(ns, k, None)
        if isinstance(v, str) and isinstance(cur, bool):
            v = str_to_bool(v)
        setattr(ns, k, v)
    return ns


TITLES = {1: "GAN_", 2: "LSGAN_", 3: "WGANGP_", 4: "HingeGAN_", 5: "RSGAN_", 6: "RaSGAN_", 7: "RaLSGAN_",
          8: "RaHingeGAN_"}
