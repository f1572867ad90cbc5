"""The five analysis programs (voice_synth_amd/cli: acoustic, formants, glottal, vtrack, vinverse) on a stand-in device,
against a recording of what they print, write and return.

tests/c/test_cli_trace.c is a program's source with main renamed, the library's real host side, the stand-in HIP runtime
and stand-in launchers whose results are a hash of everything they were given.  Each is built here under ASan/UBSan and
run, a child process per case, on input files made from a fixed seed: every option at and off its default, every refusal
of the parsers, files that are missing, truncated, not 16-bit PCM, empty or odd, batches of mixed lengths and rates, the
printers' switches, the filter tools' glides and models, VS_ARITH / VS_DEVICE, and runtime calls that fail.  Per case the
command line, the exit status, stdout, stderr and size and sha256 of the output file are compared with
tests/golden/cli_trace.txt byte for byte, with leak detection on.

    python tests/test_cli_trace.py --record

writes the recording from the programs of the working tree, with leak detection off.  It cannot see the kernels: what they
make of the same arguments is held by the GPU tests of each program."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

from test_host_sanitizers import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_trace.txt")
PROGRAMS = ("acoustic", "glottal", "formants", "vtrack", "vinverse")
HOST_UNITS = ["vs_api.c", "vs_blocks.c", "vs_planhost.c", "vs_host.c"] + [
    "vs_%s_host.c" % f for f in ("acoustic", "glottal", "lpc", "iaif", "track", "inverse")]


def build(out_dir):
    """the library's host side once, then one executable per program; {program: path}"""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    flags = ["gcc", "-std=gnu11"] + SAN + ["-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                                           "-I" + os.path.join(ROOT, "include")]
    objs = []
    jobs = []
    for unit in HOST_UNITS:
        objs.append(os.path.join(out_dir, unit[:-2] + ".o"))
        jobs.append(subprocess.Popen(flags + ["-c", os.path.join(ROOT, "voice_synth_amd", "csrc", unit), "-o", objs[-1]]))
    assert all(j.wait() == 0 for j in jobs)
    exes = {}
    jobs = []
    for prog in PROGRAMS:
        exes[prog] = os.path.join(out_dir, prog)
        jobs.append(subprocess.Popen(flags + ["-DCLI_SOURCE=\"../../voice_synth_amd/cli/%s.c\"" % prog,
                                              os.path.join(ROOT, "tests", "c", "test_cli_trace.c")] + objs +
                                     ["-o", exes[prog], "-lm", "-lpthread"]))
    assert all(j.wait() == 0 for j in jobs)
    return exes


# ---- the input files ----

def header(layout, fs, n_bytes, tag=1, bits=16):
    """the two layouts of csrc/vs_host.c's vs_wav_header_write"""
    if layout == 44:
        return (b"RIFF" + struct.pack("<I", n_bytes + 36) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, tag, 1, fs, 2 * fs, 2, bits) +
                b"data" + struct.pack("<I", n_bytes))
    return (b"RIFF\0\0\0\0" + struct.pack("<Q", n_bytes + 36) + b"WAVEfmt " + struct.pack("<QHH4xQQHH", 16, tag, 1, fs, 2 * fs, 2, bits) +
            b"data" + struct.pack("<Q", n_bytes))


def samples(seed, n):
    """int16 from a fixed linear congruential stream"""
    out, s = bytearray(), seed
    for _ in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out += struct.pack("<h", ((s >> 40) & 0xFFFF) - 32768)
    return bytes(out)


def write_inputs(d):
    a = samples(1, 2000)
    files = {
        "a.wav": header(44, 16000, len(a)) + a,
        "a72.wav": header(72, 16000, len(a)) + a,                 # the same payload behind the LP64 header
        "b.wav": header(44, 8000, 2406) + samples(2, 1203),
        "c.wav": header(72, 22050, 8000) + samples(3, 4000),
        "lo.wav": header(44, 400, 600) + samples(4, 300),         # a rate the lag range and the LPC window refuse
        "short.wav": header(44, 16000, 400) + samples(5, 200),    # no room for one 25 ms frame
        "two.wav": header(44, 16000, 4) + samples(6, 2),
        "trunc.wav": header(44, 16000, len(a))[:30],
        "tag3.wav": header(44, 16000, len(a), tag=3) + a,
        "bits8.wav": header(44, 16000, len(a), bits=8) + a,
        "empty.wav": header(44, 16000, 0),
        "empty72.wav": header(72, 16000, 0),
        "odd.wav": header(44, 16000, len(a) + 1) + a + b"\x7f",   # a trailing byte that is no sample
    }
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    return files


# ---- the cases: (program, arguments, environment) ----

BAD_NUMBERS = ["x", "", "1x", "nan", "inf", "-inf", "1e999"]


def cases():
    out = []

    def add(prog, args, **env):
        out.append((prog, args.split(" ") if isinstance(args, str) and args else (args or []), env))

    def numeric(prog, letter, tail, values, lead=""):
        """a numeric option: nothing behind it, what is no finite number, then the values given"""
        lead = lead.split(" ") if lead else []
        out.append((prog, lead + ["-" + letter], {}))
        for v in BAD_NUMBERS + values:
            out.append((prog, lead + ["-" + letter, v] + (tail.split(" ") if tail else []), {}))

    bad_files = "a.wav missing.wav trunc.wav b.wav tag3.wav bits8.wav empty.wav odd.wav a72.wav c.wav"

    # acoustic
    add("acoustic", "")
    add("acoustic", "a.wav")
    add("acoustic", "a72.wav")
    add("acoustic", "-m a.wav")
    add("acoustic", "a.wav b.wav c.wav")
    add("acoustic", "-m c.wav a.wav b.wav")
    add("acoustic", "-m -f 60 -F 400 a.wav b.wav")
    add("acoustic", bad_files)
    add("acoustic", "-m " + bad_files)
    add("acoustic", "missing.wav")
    add("acoustic", "trunc.wav tag3.wav")
    add("acoustic", "lo.wav")
    add("acoustic", "a.wav lo.wav b.wav")
    add("acoustic", "-f 20 a.wav")
    add("acoustic", "-f 5 a.wav b.wav")
    add("acoustic", "-F 9000 a.wav c.wav")
    add("acoustic", "-f 300 -F 200 a.wav")
    add("acoustic", "-m two.wav empty.wav")
    add("acoustic", "-z a.wav")
    add("acoustic", "-fx 60 a.wav")
    add("acoustic", "-m")
    add("acoustic", "- a.wav")
    numeric("acoustic", "f", "a.wav", ["0", "-5", "60", "75.5"])
    numeric("acoustic", "F", "a.wav", ["0", "-5", "400"])
    add("acoustic", "a.wav", VS_DEVICE="1")
    add("acoustic", "a.wav", VS_DEVICE="2")
    add("acoustic", "a.wav", VS_ARITH="fma")
    for k in (1, 2, 5, 9, 14, 18, 22, 23):            # the last runtime call whose failure the program sees, and one past it
        add("acoustic", "-m a.wav b.wav", VS_STANDIN_FAIL_AT=str(k))

    # glottal
    add("glottal", "")
    add("glottal", "a.wav")
    add("glottal", "a72.wav")
    add("glottal", "-c a.wav")
    add("glottal", "a.wav b.wav c.wav")
    add("glottal", "-c c.wav a.wav b.wav")
    add("glottal", "-c -f 60 -F 400 -p -1 -l 10 -L 200 a.wav b.wav")
    add("glottal", bad_files)
    add("glottal", "-c " + bad_files)
    add("glottal", "missing.wav")
    add("glottal", "lo.wav")
    add("glottal", "a.wav lo.wav b.wav")
    add("glottal", "-f 20 a.wav")
    add("glottal", "-f 5 a.wav b.wav")
    add("glottal", "-F 9000 a.wav c.wav")
    add("glottal", "-l 200 -L 100 a.wav")
    add("glottal", "-l 128 a.wav")
    add("glottal", "-l 129 a.wav")
    add("glottal", "-c two.wav empty.wav")
    add("glottal", "-z a.wav")
    add("glottal", "-fx 60 a.wav")
    add("glottal", "-c")
    numeric("glottal", "f", "a.wav", ["0", "-5", "60"])
    numeric("glottal", "F", "a.wav", ["0", "-5", "400"])
    numeric("glottal", "p", "a.wav", ["1", "-1", "0", "2", "0.5"])
    numeric("glottal", "l", "a.wav", ["0", "26", "100", "-1", "256", "1.5"])
    numeric("glottal", "L", "a.wav", ["255", "128", "26", "25", "-1", "256", "127.5"])
    add("glottal", "-c a.wav", VS_DEVICE="1")
    for k in (1, 2, 5, 9, 12, 16, 21, 26, 27):
        add("glottal", "-c a.wav b.wav", VS_STANDIN_FAIL_AT=str(k))

    # formants
    add("formants", "")
    add("formants", "a.wav")
    add("formants", "a72.wav")
    add("formants", "a.wav b.wav c.wav")
    add("formants", "-f c.wav a.wav b.wav")
    add("formants", "-c a.wav b.wav c.wav")
    add("formants", "-c -f a.wav b.wav")
    add("formants", "-n 0 a.wav b.wav")
    add("formants", "-n 0 -f -c a.wav")
    add("formants", "-t 0 a.wav b.wav")
    add("formants", "-t 0 -f a.wav")
    add("formants", "-p a.wav")
    add("formants", "-r a.wav")
    add("formants", "-p -r -f -o 10 -w 20 -t 5 -n 3 a.wav b.wav")
    add("formants", "-I a.wav b.wav")
    add("formants", "-I -f -c a.wav")
    add("formants", "-I -g 6 -l 0.9 -o 18 -n 4 -r a.wav c.wav")
    add("formants", "-I -p a.wav")
    add("formants", "-g 4 a.wav")
    add("formants", "-l .5 a.wav")
    add("formants", "-I -g 30 a.wav")
    add("formants", "-I -g 22 a.wav")
    add("formants", "-I -o 3 a.wav")
    add("formants", bad_files)
    add("formants", "-f " + bad_files)
    add("formants", "missing.wav")
    add("formants", "lo.wav")
    add("formants", "a.wav lo.wav b.wav")
    add("formants", "-w 2000 a.wav b.wav")
    add("formants", "-w 1 a.wav")
    add("formants", "short.wav two.wav empty.wav")
    add("formants", "-c short.wav a.wav")
    add("formants", "-z a.wav")
    add("formants", "-ox 10 a.wav")
    add("formants", "-c")
    numeric("formants", "o", "a.wav", ["1", "40", "0", "41", "-3", "2.5"])
    numeric("formants", "w", "a.wav", ["10", "0", "-1"])
    numeric("formants", "t", "a.wav", ["5", "0", "-1", "1e-3"])
    numeric("formants", "n", "a.wav", ["0", "1", "20", "21", "-1", "1.5"])
    numeric("formants", "g", "a.wav", ["1", "6", "0", "41", "2.5"], lead="-I")
    numeric("formants", "l", "a.wav", ["0", "1", "0.5", "1.5", "-0.1"], lead="-I")
    add("formants", "-c a.wav", VS_DEVICE="1")
    for k in (1, 2, 5, 9, 14, 20, 25, 26):
        add("formants", "-c a.wav b.wav", VS_STANDIN_FAIL_AT=str(k))
    add("formants", "-I a.wav b.wav", VS_STANDIN_FAIL_AT="9")

    # vtrack and vinverse: what the two share
    for prog in ("vtrack", "vinverse"):
        io = "-i a.wav -o out.wav"
        add(prog, "")
        add(prog, io + " -v a,i")
        add(prog, "-i a72.wav -o out.wav -v a,i")
        add(prog, io + " -v a,i,u")
        add(prog, io + " -v a,i,u,e,o,a,i")
        add(prog, "-i two.wav -o out.wav -v a,i")
        add(prog, "-i two.wav -o out.wav -v a,i,u")
        add(prog, "-i b.wav -o out.wav -v u,a")
        add(prog, io + " -v a")
        add(prog, io + " -v a,")
        add(prog, io + " -v a,,i")
        add(prog, io + " -v ?")
        add(prog, io + " -v ai")
        add(prog, io + " -v ,a")
        add(prog, [*io.split(" "), "-v", ""])
        add(prog, io + " -v " + ",".join("aiueo"[k % 5] for k in range(64)))
        add(prog, io + " -v " + ",".join("aiueo"[k % 5] for k in range(65)))
        add(prog, io + " -m c.wav")
        add(prog, io + " -m a.wav")
        add(prog, io + " -m c.wav -G")
        add(prog, "-i a72.wav -o out.wav -m b.wav -G")
        add(prog, io + " -m c.wav -O 18 -t 5")
        add(prog, io + " -G -v a,i")
        add(prog, io + " -m short.wav")
        add(prog, io + " -m two.wav -G")
        add(prog, io + " -m lo.wav")
        add(prog, io + " -m empty.wav")
        add(prog, io + " -m missing.wav")
        add(prog, io + " -m trunc.wav")
        add(prog, io + " -v a,i -m c.wav")
        add(prog, io)
        add(prog, "-o out.wav -v a,i")
        add(prog, "-i a.wav -v a,i")
        add(prog, "-i empty.wav -o out.wav -v a,i")
        add(prog, "-i empty72.wav -o out.wav -m c.wav")
        add(prog, "-i odd.wav -o out.wav -v a,i")
        add(prog, "-i a.wav -o nowhere/out.wav -v a,i")
        add(prog, "-i a.wav -o nowhere/out.wav -m c.wav")
        for name in ("missing.wav", "trunc.wav", "tag3.wav", "bits8.wav"):
            add(prog, "-i %s -o out.wav -v a,i" % name)
        add(prog, io + " -v a,i -z")
        add(prog, io + " -v a,i -z 1")
        add(prog, io + " -v a,i extra")
        add(prog, io + " -v a,i -tx 5")
        add(prog, "-i")
        add(prog, io + " -v")
        add(prog, io + " -m")
        numeric(prog, "t", "", ["5", "0", "-1"], lead=io + " -m c.wav")
        numeric(prog, "O", "", ["1", "40", "0", "41", "2.5"], lead=io + " -m c.wav")
        add(prog, io + " -v a,i -t 5 -O 18")
        add(prog, io + " -v a,i", VS_ARITH="fma")
        add(prog, io + " -m c.wav", VS_ARITH="fma")
        add(prog, io + " -v a,i", VS_ARITH="exact")
        add(prog, io + " -v a,i", VS_DEVICE="1")
        add(prog, io + " -m c.wav", VS_DEVICE="1")
        add(prog, io + " -v a,i", VS_DEVICE="2")
        for k in (1, 2, 5, 9, 13, 18, 23, 24):
            add(prog, io + " -v a,i", VS_STANDIN_FAIL_AT=str(k))
        for k in list(range(1, 50, 3)) + [41, 42, 50, 51]:  # (a release that fails goes unseen: status 0)
            add(prog, io + " -m c.wav -G", VS_STANDIN_FAIL_AT=str(k))

    # vtrack's own letters
    io = "-i a.wav -o out.wav"
    add("vtrack", io + " -v a,i -g 2.5 -p 0.9")
    add("vtrack", io + " -m c.wav -g 0.5 -p 1")
    add("vtrack", io + " -v a,i -g -3 -p -2")
    numeric("vtrack", "g", "", ["0", "10"], lead=io + " -v a,i")
    numeric("vtrack", "p", "", ["0", "1", "5"], lead=io + " -v a,i")
    add("vtrack", io + " -v a,i -P")
    add("vtrack", io + " -v a,i -I")
    add("vtrack", io + " -v a,i -s 2")

    # vinverse's own letters
    add("vinverse", io + " -v a -s 0.1 -d 0.9")
    add("vinverse", "-i two.wav -o out.wav -v a")
    add("vinverse", io + " -v a,i -s 0.1 -d 0.9")
    add("vinverse", io + " -m c.wav -s -2 -d 1")
    add("vinverse", io + " -m c.wav -P")
    add("vinverse", io + " -m c.wav -P -G -O 30")
    add("vinverse", io + " -v a,i -P")
    add("vinverse", io + " -m c.wav -I")
    add("vinverse", io + " -m a.wav -I -G")
    add("vinverse", io + " -m c.wav -I -g 6 -l 0.9")
    add("vinverse", io + " -m c.wav -I -g 6 -l 0.9 -O 18 -t 5 -G -s 0.5 -d 0.5")
    add("vinverse", io + " -m short.wav -I")
    add("vinverse", io + " -I -v a")
    add("vinverse", io + " -I -v a,i")
    add("vinverse", io + " -m c.wav -I -P")
    add("vinverse", io + " -m c.wav -l .5")
    add("vinverse", io + " -m c.wav -g 4")
    add("vinverse", io + " -m c.wav -I -g 30")
    add("vinverse", io + " -m c.wav -I -O 3")
    add("vinverse", io + " -m c.wav -I -O 4")
    numeric("vinverse", "s", "", ["0", "-1", "10"], lead=io + " -v a,i")
    numeric("vinverse", "d", "", ["0", "1", "0.5", "1.5", "-0.1"], lead=io + " -v a,i")
    numeric("vinverse", "g", "", ["1", "6", "0", "41", "2.5"], lead=io + " -m c.wav -I")
    numeric("vinverse", "l", "", ["0", "1", "0.5", "1.5", "-0.1"], lead=io + " -m c.wav -I")
    add("vinverse", io + " -m c.wav -I", VS_ARITH="fma", VS_DEVICE="1")
    for k in (5, 9, 14, 20, 30, 36, 38, 39, 44, 50):
        add("vinverse", io + " -m c.wav -I", VS_STANDIN_FAIL_AT=str(k))
    return out


# ---- running and writing down ----

KEEP_LINES, KEEP_COLUMNS = 6, 160  # a longer text: its first lines and a hash of all of it; a longer line likewise


def output_of(args):
    for k, a in enumerate(args[:-1]):
        if a == "-o":
            return args[k + 1]
    return None


def run_case(exes, d, inputs, usage, case, leaks):
    prog, args, env = case
    out_name = output_of(args)
    out_path = os.path.join(d, out_name) if out_name else None
    if out_path and os.path.exists(out_path):
        os.remove(out_path)
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("VS_")}
    child_env.update(env, ASAN_OPTIONS="detect_leaks=%d" % leaks, UBSAN_OPTIONS="print_stacktrace=0")
    r = subprocess.run([exes[prog]] + args, cwd=d, env=child_env, capture_output=True, timeout=120)
    head = "== " + " ".join([k + "=" + env[k] for k in sorted(env)] + [prog] + [a if a else "''" for a in args])
    lines = [head, "status %d" % r.returncode]
    for name, text in (("stdout", r.stdout), ("stderr", r.stderr)):
        if name == "stderr" and text and text == usage.get(prog):
            lines.append("stderr: the usage line")
            continue
        text_lines = text.decode("latin-1").split("\n")
        if text_lines[-1] == "":
            text_lines.pop()                          # (a last line without its newline would show as one more case)
        for l in text_lines[:KEEP_LINES] if len(text_lines) > 2 * KEEP_LINES else text_lines:
            lines.append("%s| %s" % (name, l if len(l) <= KEEP_COLUMNS else "%s... %d characters, sha256 %s" % (
                l[:KEEP_COLUMNS], len(l), hashlib.sha256(l.encode("latin-1")).hexdigest()[:16])))
        if len(text_lines) > 2 * KEEP_LINES:
            lines.append("%s: %d lines in all, sha256 %s" % (name, len(text_lines), hashlib.sha256(text).hexdigest()[:32]))
    if out_name:
        if os.path.exists(out_path):
            with open(out_path, "rb") as f:
                data = f.read()
            in_name = args[args.index("-i") + 1] if "-i" in args[:-1] else None
            src = inputs.get(in_name, b"")
            hbytes = 72 if src[16:20] == b"WAVE" else 44
            same = "the input's" if data[:hbytes] == src[:hbytes] else "NOT the input's"
            lines.append("file %s: %d bytes, sha256 %s, header %s" % (out_name, len(data), hashlib.sha256(data).hexdigest()[:32], same))
        else:
            lines.append("file %s: absent" % out_name)
    if prog not in usage:  # the program's first case: no arguments
        usage[prog] = r.stderr
    return "\n".join(lines) + "\n"


def trace(work_dir, leaks):
    exes = build(work_dir)
    d = os.path.join(work_dir, "run")
    os.mkdir(d)
    inputs = write_inputs(d)
    usage = {}
    return [run_case(exes, d, inputs, usage, c, leaks) for c in cases()]


def test_cli_boundary_trace(tmp_path):
    got = trace(str(tmp_path), leaks=1)
    with open(GOLDEN, "rb") as f:
        want = f.read().decode("latin-1")
    if "".join(got) == want:
        return
    want_cases = ["== " + c for c in want.split("\n== ")]  # which case differs, for the message
    want_cases[0] = want_cases[0][3:]
    want_cases = [c if c.endswith("\n") else c + "\n" for c in want_cases]
    assert len(got) == len(want_cases), "the recording holds %d cases, the table %d" % (len(want_cases), len(got))
    wrong = [(g, w) for g, w in zip(got, want_cases) if g != w]
    assert not wrong, "%d of %d cases differ from the recording; the first:\n--- got\n%s--- recorded\n%s" % (
        len(wrong), len(got), wrong[0][0], wrong[0][1])
    raise AssertionError("the trace differs from the recording between its cases")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_cli_trace.py --record")
    with tempfile.TemporaryDirectory() as work:
        text = "".join(trace(work, leaks=0))
    with open(GOLDEN, "wb") as f:
        f.write(text.encode("latin-1"))
    print("%s: %d cases, %d bytes" % (GOLDEN, text.count("\n== ") + 1, len(text)))
