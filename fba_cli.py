#!/usr/bin/env python3
"""Command line for the reference's two entry points on the MI355X path:

    python fba_cli.py main <folder> [plot] [--reliability]     main(folder, plot)  (main.m:10);
                                               --reliability also writes the .rel table (report.write_rel)
    ... main <folder> ... --ellipsoids         also writes the .ell table (report.write_ell): every tie point's
                                               sigma X Y Z, 1-sigma error ellipsoid and horizontal error ellipse
    ... main <folder> ... --intersect          the tie points' starting values by forward intersection of their image
                                               rays instead of the .cnt coordinates; also writes the .fwd table
                                               (report.write_fwd)
    ... main <folder> ... --resect[=control|all]  the images' starting values by space resection from their control
                                               points (all: and the tie points at their .cnt coordinates) instead of
                                               the .ext values; also writes the .rsc table (report.write_rsc)
    ... main <folder> ... --vce[=xy|camera|camera_xy]  variance components of the image measurements per axis (the
                                               default), per camera or per camera and axis, estimated and applied
                                               on the device before the post-fit outputs; also writes the .vce table
                                               (report.write_vce); not together with --robust
    ... main <folder> ... --snoop[=crit]       Baarda data snooping: the image points whose w-test exceeds crit (3.29)
                                               are eliminated on the device round by round and re-checked at the end;
                                               also writes the .snp table (report.write_snp); --reliability then shows
                                               the cleaned block; not together with --robust
    python fba_cli.py batch <folder>...        BatchRun.m without its folder picker
    ... --robust huber[:k] | cauchy[:k]        (either command) robust loss after the L2 iterations, k in units
                                               of sigma (default: the 95 %-efficiency constants, huber 1.345,
                                               cauchy 2.385); also writes the .wgt table (report.write_wgt)
    ... --priors                               (either command) the folder's .pri table, rows `<unknown name>
                                               <value> <std>`, as prior observations of unknowns; also writes
                                               the .prr table (report.write_prr)
    ... --lm[=lambda0]                         (either command) Levenberg-Marquardt trials with step control, then
                                               undamped passes, in place of the Gauss-Newton loop (first lambda
                                               1e-3): for coarse starting values; also writes the .lm table
                                               (report.write_lm)
"""
import sys

import fba_import

if __name__ == "__main__":
    fba = fba_import.load()
    from fba_amd.batch import cli
    sys.exit(cli())
