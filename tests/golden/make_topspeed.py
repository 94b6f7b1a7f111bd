"""Generates tests/golden/topspeed_windowing.json: the input and the expected output of the TopSpeedWindowing example
(flink-examples/flink-examples-streaming/src/main/java/org/apache/flink/streaming/examples/windowing/
TopSpeedWindowing.java:71-87: keyBy(0).window(GlobalWindows).evictor(TimeEvictor.of(10 s)).trigger(DeltaTrigger.of(50,
new.f2 - old.f2)).maxBy(1)) as number tuples (car id, speed, distance, timestamp):
  CAR_DATA    util/TopSpeedWindowingExampleData.java:25-125, parsed as TopSpeedWindowing.ParseCarData does (:144-153);
  TOP_SPEEDS  util/TopSpeedWindowingExampleData.java:127-198, the rows TopSpeedWindowingExampleITCase.java:50-62
              compares with the job's output as sorted lines.
Run where the reference checkout exists (REFERENCE_ROOT, default /root/reference); the JSON is the committed data
fixture the tests read.
"""
import json
import os
import re

REL = ("flink-examples/flink-examples-streaming/src/main/java/org/apache/flink/streaming/examples/windowing/util/"
       "TopSpeedWindowingExampleData.java")
SRC = os.path.join(os.environ.get("REFERENCE_ROOT", "/root/reference"), REL)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "topspeed_windowing.json")


def _tuples(lines, name):
    """(first line, last line, tuples) of the String constant `name`"""
    first = next(i for i, ln in enumerate(lines) if f"String {name} =" in ln)
    last = next(i for i in range(first, len(lines)) if lines[i].rstrip().endswith(";"))
    body = "".join(lines[first:last + 1])
    out = []
    for m in re.findall(r"\((\d+),(\d+),([0-9.eE+-]+),(\d+)\)", body):
        out.append([int(m[0]), int(m[1]), float(m[2]), int(m[3])])  # Integer, Integer, Double.valueOf, Long
    return first + 1, last + 1, out


def main():
    lines = open(SRC).read().split("\n")
    a0, a1, cars = _tuples(lines, "CAR_DATA")
    b0, b1, tops = _tuples(lines, "TOP_SPEEDS")
    json.dump({"source": {"CAR_DATA": f"TopSpeedWindowingExampleData.java:{a0}-{a1}",
                          "TOP_SPEEDS": f"TopSpeedWindowingExampleData.java:{b0}-{b1}",
                          "job": "TopSpeedWindowing.java:71-87", "compared": "TopSpeedWindowingExampleITCase.java:50-62"},
               "fields": ["car", "speed", "distance", "timestamp"],
               "threshold": 50.0, "evictor_ms": 10000,
               "CAR_DATA": cars, "TOP_SPEEDS": tops}, open(OUT, "w"), indent=0)
    print(len(cars), "records,", len(tops), "expected rows")


if __name__ == "__main__":
    main()
