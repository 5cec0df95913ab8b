"""Trains a Knn model on hashed term-frequency vectors (HashingTF's 262,144-wide sparse output) and
classifies new documents with it. The sparse feature column is never densified when it takes the
CSR route (``FMLX_KNN_CSR``: ``1`` always, ``auto`` by size and density, ``0`` never); the model
data then holds the CSR training set (``CsrPackedFeatures``).

Run: FMLX_KNN_CSR=1 python examples/classification/knn_sparse_example.py
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from flink_ml_amd import Table  # noqa: E402
from flink_ml_amd.lib.classification.knn import KNN  # noqa: E402
from flink_ml_amd.lib.feature import HashingTF  # noqa: E402

docs = [("the gpu kernel runs a wave of threads", 1.0), ("a kernel launch fills the gpu with waves", 1.0),
        ("threads of a wave share the lds", 1.0), ("the gpu runs the kernel on every compute unit", 1.0),
        ("knead the dough and let the bread rise", 2.0), ("bake the bread until the crust is brown", 2.0),
        ("the dough needs flour water and salt", 2.0), ("let the dough rest then bake it", 2.0)]
queries = [("how many threads does a gpu wave have", 1.0), ("how long should bread dough rise", 2.0)]

tf = HashingTF().set_input_col("words").set_output_col("features")
train = tf.transform(Table.from_rows([(d.split(), y) for d, y in docs], ["words", "label"]))[0]
test = tf.transform(Table.from_rows([(d.split(), y) for d, y in queries], ["words", "label"]))[0]
model = KNN().set_k(3).fit(train)
packed = model.get_model_data()[0].column("packedFeatures")[0]
print("Model data: %s of %d x %d" % (type(packed).__name__, packed.num_rows, packed.num_cols))
out = model.transform(test)[0]
for words, label, pred in zip(out.get_list("words"), out.get_list("label"), out.get_list("prediction")):
    print("Document: %s \tExpected Result: %s \tPrediction Result: %s" % (" ".join(words), label, pred))
