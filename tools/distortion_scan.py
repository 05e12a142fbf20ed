"""Find the coefficient of --distortion-correction: stitch one region once per candidate D with --seam-qc and print, per D, the
median zero-normalised cross-correlation of the seams at their best offset and the number of seams flagged `shifted`.  Radial
distortion displaces the two sides of a seam against each other by an amount that changes along the seam, which no placement
removes: the D that undoes it has the highest median and the fewest shifted seams.

    python tools/distortion_scan.py -i /path/to/acquisition [-r] [--region R0] [--timepoint 0] [--radius 2] -- -3000 -1500 0 1500 3000

Nothing is kept: the region is fused in memory and the reports go to a temporary folder that is removed."""
import argparse
import shutil
import statistics
import sys
import tempfile

sys.path.insert(0, '.')
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters


def scan(input_folder, values, region=None, timepoint=None, use_registration=False, radius=2, **stitcher_options):
    """[(D, median best ncc or None, shifted seams, measured seams)] for every D of ``values``."""
    found = []
    for ppm in values:
        out = tempfile.mkdtemp(prefix='distortion_scan_')
        try:
            st = Stitcher(StitchingParameters(input_folder=input_folder, use_registration=use_registration), seam_qc=True,
                          seam_qc_radius=radius, distortion_correction=ppm, **stitcher_options)
            st.output_folder = out
            st.get_timepoints()
            st.extract_acquisition_parameters()
            st.get_pixel_size()
            st.parse_acquisition_metadata()
            t = st.timepoints[0] if timepoint is None else timepoint
            r = st.regions[0] if region is None else region
            if use_registration:
                st.calculate_shifts(t, r)
            st.stitch_region(t, r)
            rows = [row for row in st.seam_qc_table[(int(t), r)] if row['best_ncc'] is not None]
            shifted = sum('shifted' in row['flags'].split('|') for row in rows)
            found.append((ppm, statistics.median(row['best_ncc'] for row in rows) if rows else None, shifted, len(rows)))
        finally:
            shutil.rmtree(out, ignore_errors=True)
    return found


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('-i', '--input-folder', required=True)
    parser.add_argument('-r', '--use-registration', action='store_true')
    parser.add_argument('--region', default=None)
    parser.add_argument('--timepoint', type=int, default=None)
    parser.add_argument('--radius', type=int, default=2, help="--seam-qc-radius of the runs, 0..3")
    parser.add_argument('values', type=int, nargs='+', metavar='D', help="candidates in parts per million, -50000..50000")
    args = parser.parse_args(argv)
    found = scan(args.input_folder, args.values, args.region, args.timepoint, args.use_registration, args.radius)
    print(f"{'D (ppm)':>9}  {'median best ncc':>16}  {'shifted':>8}  {'seams':>6}")
    for ppm, ncc, shifted, n in found:
        print(f"{ppm:>9}  {'-' if ncc is None else format(ncc, '.6f'):>16}  {shifted:>8}  {n:>6}")
    measured = [f for f in found if f[1] is not None]
    if measured:
        best = max(measured, key=lambda f: (f[1], -f[2]))
        print(f"highest median: D = {best[0]}")
    return found


if __name__ == '__main__':
    main()
