"""Batch driver: BatchRun.m without the folder-picker GUI.

``find_folders`` restates BatchRun.m's ``findfiles`` (BatchRun.m:71-150): a folder qualifies when it
holds one each of .pho/.ext/.cnt/.int; a folder holding some but not all of them is reported and
skipped; a second file of an extension already seen prints a warning and clears the list of found
extensions (the reference's ``found = []``, BatchRun.m:92-96); subfolders are searched recursively
after the folder's own files.  ``batch_run`` calls ``main(folder)`` for each qualifying folder in order
and stops at the first failure (BatchRun.m:56-64).
"""
import os
import sys

EXTS = (".pho", ".ext", ".cnt", ".int")


def _join(items):
    return ", ".join(items[:-1]) + " and " + items[-1] if len(items) > 1 else items[0]


def find_folders(folder, exts=EXTS, log=print):
    """BatchRun.m:71-150 (files in name order, as MATLAB's dir lists them)."""
    out = []
    try:
        entries = sorted(os.listdir(folder))
    except OSError:
        return out
    files = [e for e in entries if os.path.isfile(os.path.join(folder, e))]
    if files:
        found = []
        for name in files:
            ext = os.path.splitext(name)[1]
            if ext in exts:
                if ext in found:
                    log(f"Warning: More than 1 {ext} file was found in {folder}")
                    found = []
                found.append(ext)
        if found and len(found) < len(exts):
            missing = [e for e in sorted(exts) if e not in found]  # setdiff returns sorted values
            log(f'Error: {_join(found)} {"were" if len(found) > 1 else "was"} found in "{folder}" but not '
                f"{_join(missing)}. This folder will be skipped")
        elif len(found) == len(exts):
            out.append(folder)
    for name in entries:
        sub = os.path.join(folder, name)
        if os.path.isdir(sub):
            out.extend(find_folders(sub, exts, log))
    return out


def batch_run(paths, device=0, robust=None, robust_k=None, priors=False, lm=None):
    """BatchRun.m:42-66: every data folder under the selected paths through main(folder, false);
    stops at the first folder whose main() fails.  Returns the list of (folder, main_error).
    robust / robust_k: the robust loss of bundle.adjust, for every folder; priors: every folder's .pri table;
    lm: parse_lm's value, the damped loop (method="lm") for every folder."""
    from .bundle import main
    folders = []
    for p in paths:
        folders.extend(find_folders(p))
    done = []
    for f in folders:
        err = main(f, False, device=device, **_robust_kw(robust, robust_k), **_priors_kw(priors), **_lm_kw(lm))
        done.append((f, err))
        if err == 1:
            break
    return done


def _robust_kw(robust, robust_k):
    """main()'s keywords for a robust loss; none without one, so the call is the one it was"""
    return {"robust": robust, "robust_k": robust_k} if robust else {}


def _priors_kw(priors):
    """main()'s keyword for the .pri table; none without it, so the call is the one it was"""
    return {"priors": True} if priors else {}


def _lm_kw(lm):
    """main()'s keywords for the damped loop (lm: None, True or lambda0); none without it, so the call is the one
    it was"""
    if lm is None or lm is False:
        return {}
    return {"method": "lm", "lm_options": None if lm is True else {"lambda0": float(lm)}}


def parse_lm(args):
    """--lm or --lm=lambda0 anywhere in args -> (args without it, None / True / lambda0): Levenberg-Marquardt
    trials with step control in place of the Gauss-Newton loop.  ValueError for a lambda0 that is not a positive
    number."""
    rest, lm = [], None
    for a in args:
        if a == "--lm":
            lm = True
        elif a.startswith("--lm="):
            lm = float(a.split("=", 1)[1])
            if not (lm > 0.0 and lm < float("inf")):
                raise ValueError("--lm: lambda0 must be a positive number")
        else:
            rest.append(a)
    return rest, lm


def parse_priors(args):
    """--priors anywhere in args -> (args without it, True / False): use the folder's .pri table"""
    return [a for a in args if a != "--priors"], "--priors" in args


def parse_ellipsoids(args):
    """--ellipsoids anywhere in args -> (args without it, True / False): the tie points' full covariance blocks
    and error ellipsoids (`main` only; writes the .ell table)"""
    return [a for a in args if a != "--ellipsoids"], "--ellipsoids" in args


def parse_intersect(args):
    """--intersect anywhere in args -> (args without it, True / False): the tie points' starting values by forward
    intersection of their image rays (`main` only; writes the .fwd table)"""
    return [a for a in args if a != "--intersect"], "--intersect" in args


def parse_resect(args):
    """--resect, --resect=control or --resect=all anywhere in args -> (args without it, False / "control" / "all"):
    the images' starting values by space resection (`main` only; writes the .rsc table).  ValueError for another
    class."""
    rest, resect = [], False
    for a in args:
        if a == "--resect":
            resect = "control"
        elif a.startswith("--resect="):
            resect = a.split("=", 1)[1].lower()
            if resect not in ("control", "all"):
                raise ValueError("--resect: control or all")
        else:
            rest.append(a)
    return rest, resect


def parse_vce(args):
    """--vce, --vce=xy, --vce=camera or --vce=camera_xy anywhere in args -> (args without it, None or the grouping;
    a bare --vce is "xy"): variance components of the image measurements' groups (`main` only; writes the .vce table).
    ValueError for another grouping."""
    rest, vce = [], None
    for a in args:
        if a == "--vce":
            vce = "xy"
        elif a.startswith("--vce="):
            vce = a.split("=", 1)[1].lower()
            if vce not in ("xy", "camera", "camera_xy"):
                raise ValueError("--vce: xy, camera or camera_xy")
        else:
            rest.append(a)
    return rest, vce


def parse_snoop(args):
    """--snoop or --snoop=<crit> anywhere in args -> (args without it, None, True or the critical value): Baarda data
    snooping of the image points (`main` only; writes the .snp table).  ValueError for a crit that is not a positive
    number."""
    rest, snoop = [], None
    for a in args:
        if a == "--snoop":
            snoop = True
        elif a.startswith("--snoop="):
            try:
                snoop = float(a.split("=", 1)[1])
            except ValueError:
                snoop = float("nan")
            if not (snoop > 0.0 and snoop < float("inf")):
                raise ValueError("--snoop: the critical value must be a positive number")
        else:
            rest.append(a)
    return rest, snoop


def parse_robust(args):
    """--robust huber[:k] | cauchy[:k] (also --robust=...) anywhere in args -> (args without it, loss or None,
    k or None).  ValueError for a missing or unknown loss, or a k that is not a positive number."""
    rest, spec = [], None
    it = iter(args)
    for a in it:
        if a == "--robust":
            spec = next(it, None)
            if spec is None:
                raise ValueError("--robust needs huber[:k] or cauchy[:k]")
        elif a.startswith("--robust="):
            spec = a.split("=", 1)[1]
        else:
            rest.append(a)
    if spec is None:
        return rest, None, None
    loss, _, ks = spec.partition(":")
    loss = loss.lower()
    if loss not in ("huber", "cauchy"):
        raise ValueError(f"--robust: unknown loss {loss!r} (huber or cauchy)")
    k = None
    if ks:
        k = float(ks)
        if not (k > 0.0 and k < float("inf")):
            raise ValueError("--robust: k must be a positive number")
    return rest, loss, k


def parse_main(args):
    """`main`'s arguments <folder> [plot] [--reliability] -> (folder, plot, reliability); the flag may stand
    anywhere after the folder (a --robust option is parse_robust's, --priors parse_priors', --lm parse_lm's)"""
    args = parse_snoop(parse_vce(parse_resect(args)[0])[0])[0]
    args = parse_intersect(parse_ellipsoids(parse_lm(parse_priors(parse_robust(args)[0])[0])[0])[0])[0]
    rest = [a for a in args[1:] if a != "--reliability"]
    return args[0], bool(rest) and rest[0] not in ("0", "false"), "--reliability" in args[1:]


USAGE = ("usage: fba_cli.py main <folder> [plot] [--reliability] [--ellipsoids] [--intersect] [--resect[=control|all]] [--vce[=xy|camera|camera_xy]] [--snoop[=crit]] [--robust LOSS[:k]] [--priors] [--lm[=lambda0]] | "
         "batch <folder>... [--robust LOSS[:k]] [--priors] [--lm[=lambda0]]\n  --robust huber[:k] | cauchy[:k]  robust loss after the L2 iterations, "
         "re-weighted at every linearisation;\n      k in units of sigma, default the 95 %-efficiency constant: huber "
         "1.345, cauchy 2.385; writes the .wgt table\n  --priors  the folder's .pri table (<unknown name> <value> "
         "<std> per row) as prior observations of unknowns;\n      writes the .prr table\n  --lm[=lambda0]  "
         "Levenberg-Marquardt trials with step control (first lambda 1e-3), then undamped passes, in place of\n"
         "      the Gauss-Newton loop: for coarse starting values; writes the .lm table\n  --ellipsoids  (main) every tie "
         "point's full 3 x 3 covariance and 1-sigma error ellipsoid; writes the .ell table\n  --intersect  (main) the tie "
         "points' starting values by forward intersection of their image rays instead of the .cnt\n      coordinates; "
         "writes the .fwd table\n  --resect[=control|all]  (main) the images' starting values by space resection from their control "
         "points (all: and\n      the tie points at their .cnt coordinates) instead of the .ext values; writes the .rsc "
         "table\n  --vce[=xy|camera|camera_xy]  (main) variance components of the image measurements per axis, per camera or "
         "per camera and\n      axis, estimated and applied before the post-fit outputs (not with --robust); writes the "
         ".vce table\n  --snoop[=crit]  (main) Baarda data snooping: image points whose w-test exceeds crit (3.29) are "
         "eliminated on the\n      device round by round and re-checked at the end (not with --robust); writes the .snp table")


def cli(argv=None):
    """python -m fba_cli main <folder> [plot] [--reliability] [--robust LOSS[:k]] [--priors] | batch <folder>...
    [--robust LOSS[:k]] [--priors]   (main(folder, plot) / BatchRun.m); LOSS huber (k = 1.345) or cauchy (k = 2.385)"""
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        argv, priors = parse_priors(argv)
        argv, lm = parse_lm(argv)
        argv, robust, robust_k = parse_robust(argv)
        argv, ellipsoids = parse_ellipsoids(argv)
        argv, intersect = parse_intersect(argv)
        argv, resect = parse_resect(argv)
        argv, vce = parse_vce(argv)
        if vce and robust:
            raise ValueError("--vce cannot be combined with --robust")
        argv, snoop = parse_snoop(argv)
        if snoop and robust:
            raise ValueError("--snoop cannot be combined with --robust")
    except ValueError as e:
        print(f"Error: {e}")
        print(USAGE)
        return 2
    if len(argv) >= 2 and argv[0] == "main":
        from .bundle import main
        folder, plot, reliability = parse_main(argv[1:])
        return main(folder, plot, reliability=reliability, **_robust_kw(robust, robust_k), **_priors_kw(priors),
                    **_lm_kw(lm), **({"ellipsoids": True} if ellipsoids else {}),
                    **({"intersect": True} if intersect else {}), **({"resect": resect} if resect else {}),
                    **({"vce": vce} if vce else {}), **({"snoop": snoop} if snoop else {}))
    if len(argv) >= 2 and argv[0] == "batch":
        done = batch_run(argv[1:], **_robust_kw(robust, robust_k), **_priors_kw(priors), **({"lm": lm} if lm else {}))
        return 1 if any(e for _, e in done) else 0
    print(USAGE)
    return 2
