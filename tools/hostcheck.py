"""What the tools/*_hostcheck.py drivers share (a helper, not a check of its own): the command line, the sanitizer flags, compiling
the driver's tools/<name>.cpp into a temporary directory, running it as a stand-alone host program and the report.  CPU only:
nothing is loaded into python and no device is touched."""
import argparse
import os
import shutil
import subprocess
import tempfile

FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COMPILERS = {"cxx": lambda: shutil.which("g++") or shutil.which("clang++") or "c++",
             "hipcc": lambda: shutil.which("hipcc") or "/opt/rocm/bin/hipcc"}


def run(script, headline, data=None, compiler="cxx", flags=(), rows_first=False):
    """Compile the ``.cpp`` beside the driver ``script`` with ``--<compiler>`` (``flags`` before the sanitizer flags), run it on a file
    that holds the bytes ``data`` (None: no file, no argument), and print -- ``--out``: also append -- ``headline`` (``{cxx}`` in it:
    the compiler's base name), the program's output and its exit code with the sanitizers' reports.  ``rows_first``: all but the last
    line of the output is printed before the headline and kept out of ``--out``.  Returns the program's exit code."""
    name = os.path.splitext(os.path.basename(script))[0]
    ap = argparse.ArgumentParser()
    ap.add_argument("--" + compiler, dest="cxx", default=COMPILERS[compiler]())
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe, argv = os.path.join(tmp, name), []
        if data is not None:
            argv = [os.path.join(tmp, "records.bin")]
            with open(argv[0], "wb") as f:
                f.write(data)
        subprocess.check_call([a.cxx, *flags, *FLAGS, os.path.splitext(os.path.abspath(script))[0] + ".cpp", "-o", exe])
        prog = subprocess.run([exe] + argv, capture_output=True, text=True)
    rows = prog.stdout.strip().splitlines() if rows_first else [prog.stdout.strip()]
    lines = [f"tools/{name}.py: " + headline.format(cxx=os.path.basename(a.cxx))] + rows[-1:] + \
            [f"exit code {prog.returncode}; sanitizer reports: {prog.stderr.strip() or 'none'}"]
    print("\n".join(rows[:-1] + lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return prog.returncode
