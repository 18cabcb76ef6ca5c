"""Writes the reference's own data files that tests/test_world_loaders.py reads, as fixtures under tests/golden/:

    python oracle/gen_reference_data_fixture.py <checkout of the reference project>

  * reference_data/validation_cases.yml, reference_data/training_cases.yml: the reference's torchdriveenv/data/*.yml, copied
    byte for byte;
  * reference_background_traffic.json.gz: every file of the reference's torchdriveenv/resources/background_traffic/ as
    {file name: document}, each document without its recurrent states (132 floats per agent that feed the remote model only,
    ref gym_env.py:216,286-287, and that loaders.load_background_traffic drops: 14 MB of the 14.7).  gzip without a
    timestamp, so the same input gives the same bytes."""
import gzip
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def main(ref):
    os.makedirs(os.path.join(OUT, "reference_data"), exist_ok=True)
    for n in ("validation_cases.yml", "training_cases.yml"):
        shutil.copyfile(os.path.join(ref, "torchdriveenv", "data", n), os.path.join(OUT, "reference_data", n))
    src = os.path.join(ref, "torchdriveenv", "resources", "background_traffic")
    docs = {}
    for n in sorted(os.listdir(src)):
        with open(os.path.join(src, n)) as f:
            doc = json.load(f)
        doc.pop("recurrent_states", None)
        docs[n] = doc
    path = os.path.join(OUT, "reference_background_traffic.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0, filename="") as f:
        f.write(json.dumps(docs, separators=(",", ":")).encode())
    print("wrote", len(docs), "background-traffic documents,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
