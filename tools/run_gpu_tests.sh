#!/bin/bash
# The GPU tests, one pytest process per file, each under a time limit of its own; the first file that fails, faults or runs
# into its limit ends the run (nothing more is started on a device that may have faulted).
# usage: tools/run_gpu_tests.sh [seconds per file] [test files ...]   (default: 600 s, every tests/test_*.py that has GPU tests)
here="$(cd "$(dirname "$0")/.." && pwd)"
cd "$here" || exit 1
limit=600
if [[ "$1" =~ ^[0-9]+$ ]]; then limit="$1"; shift; fi
files=("$@")
if [ ${#files[@]} -eq 0 ]; then
  mapfile -t files < <(grep -l "mark.gpu" tests/test_*.py | sort)
fi
for f in "${files[@]}"; do
  echo "== $f"
  timeout -k 10 "$limit" python3 -m pytest -q -m gpu -p no:cacheprovider "$f"
  rc=$?
  if [ $rc -eq 5 ]; then continue; fi  # (no GPU test selected in this file)
  if [ $rc -ne 0 ]; then echo "== $f: exit status $rc, stopping"; exit $rc; fi
done
echo "== all GPU test files passed"
