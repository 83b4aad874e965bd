"""A shape gallery: embed shapes once, keep the matrix where it is, ask for the top k of some text embeddings.

compute_metrics (eval_retrieval.py) rebuilds its matrices from per-caption tuples on every call; a ShapeGallery holds the
[Ns, D] float32 shape embeddings on the device they were given on, with the model id (and category) of every row, and ranks
queries against them:

    gallery, labels = ShapeGallery.from_captions(model_ids, categories, net.encode_shapes(batch))
    idx, sim, ids = gallery.query(net.encode_text(batch), k=5)
    idx, sim, ids, first_hit = gallery.rank(net.encode_text(batch), labels, k=5)

The order is the reference's (eval_retrieval.py:70-82): float64 dot products, larger first, equal similarities with the HIGHER shape
index first; first_hit[q] is the number of shapes ranking before shape labels[q] (MRR = mean 1 / (first_hit + 1)).  GPU tensors go
through ops.retrieval_gallery (csrc/gallery.hip): any number of shapes, k <= 64, D <= 4096.  On CPU tensors the same functions run a
float64 torch restatement of that order (a stable ascending argsort, flipped); it exists so that the interface and the ranking rule
can be used and tested without a GPU, is not tuned (it holds the whole [Nq, Ns] similarity matrix), and its similarities are torch's
matmul sums, not bit-equal to the kernel's.
"""
import numpy as np
import torch


class ShapeGallery:
    def __init__(self, embeddings, model_ids, categories=None):
        if embeddings.dim() != 2 or embeddings.dtype != torch.float32:
            raise ValueError("ShapeGallery: embeddings must be a float32 [Ns, D] tensor")
        model_ids = [str(m) for m in model_ids]
        if len(model_ids) != embeddings.shape[0]:
            raise ValueError(f"ShapeGallery: {embeddings.shape[0]} embeddings for {len(model_ids)} model ids")
        if categories is not None and len(categories) != len(model_ids):
            raise ValueError(f"ShapeGallery: {len(categories)} categories for {len(model_ids)} model ids")
        self.embeddings = embeddings.detach().contiguous()
        self.model_ids = model_ids
        self.categories = None if categories is None else [str(c) for c in categories]

    def __len__(self):
        return len(self.model_ids)

    @property
    def device(self):
        return self.embeddings.device

    @classmethod
    def from_captions(cls, model_ids, categories, shape_features, dataset=None):
        """Per-caption rows -> (gallery, labels int64 [rows]) by the rule of construct_embeddings_matrix: the FIRST row of each model id
        supplies its embedding, labels[i] is the gallery row of caption i; for dataset == "Primitives" the category is the key (and
        the model id takes the category's place).  The strings are de-duplicated on the host, the rows gathered where they are."""
        if shape_features.shape[0] != len(model_ids) or len(categories) != len(model_ids):
            raise ValueError("from_captions: model_ids, categories and shape_features must have one entry per caption")
        keys, others = (categories, model_ids) if dataset == "Primitives" else (model_ids, categories)
        label_of, first_rows = {}, []
        labels = np.zeros(len(keys), dtype=np.int64)
        for i, key in enumerate(keys):
            if key not in label_of:
                label_of[key] = len(first_rows)
                first_rows.append(i)
            labels[i] = label_of[key]
        rows = torch.tensor(first_rows, dtype=torch.int64, device=shape_features.device)
        emb = shape_features.detach().to(torch.float32).index_select(0, rows)
        return cls(emb, [keys[i] for i in first_rows], [others[i] for i in first_rows]), labels

    # ------------------------------------------------------------------------------------------------ ranking
    def _rank(self, text_features, labels, k):
        text = text_features.detach().to(torch.float32).contiguous()
        if text.dim() != 2 or text.shape[1] != self.embeddings.shape[1]:
            raise ValueError(f"ShapeGallery: queries must be [Nq, {self.embeddings.shape[1]}]")
        if text.device != self.device:
            raise ValueError(f"ShapeGallery: queries on {text.device}, gallery on {self.device}")
        if not 1 <= k <= len(self):
            raise ValueError("ShapeGallery: need 1 <= k <= number of shapes")
        lab = None
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels), dtype=torch.int64)
            if lab.shape != (text.shape[0],) or (lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= len(self))):
                raise ValueError("ShapeGallery: one label in [0, number of shapes) per query")
        if text.is_cuda:
            from .. import ops
            idx, sim, hit = ops.retrieval_gallery(text, self.embeddings, None if lab is None else lab.to(torch.int32).to(self.device), k)
            return idx.long(), sim, None if hit is None else hit.long()
        sims = text.double() @ self.embeddings.double().t()
        order = torch.flip(torch.argsort(sims, dim=1, stable=True), dims=(1,))
        top = order[:, :k].contiguous()
        hit = None if lab is None else (order == lab[:, None]).to(torch.int64).argmax(dim=1)
        return top, torch.gather(sims, 1, top), hit

    def _ids(self, idx):
        return [[self.model_ids[j] for j in row] for row in idx.cpu().tolist()]

    def query(self, text_features, k=5):
        """-> (indices [Nq,k] int64, similarities [Nq,k] float64, model ids [Nq][k]) of the k best shapes per query, best first."""
        idx, sim, _ = self._rank(text_features, None, k)
        return idx, sim, self._ids(idx)

    def rank(self, text_features, labels, k=5):
        """query() plus first_hit [Nq] int64: how many shapes rank before shape labels[q]."""
        idx, sim, hit = self._rank(text_features, labels, k)
        return idx, sim, self._ids(idx), hit

    # ------------------------------------------------------------------------------------------------ storage
    def save(self, path):
        """An .npz of embeddings (float32), model_ids and categories (strings; an empty array when there are none)."""
        with open(path, "wb") as f:
            np.savez(f, embeddings=self.embeddings.cpu().numpy(), model_ids=np.array(self.model_ids, dtype=str),
                     categories=np.array(self.categories if self.categories is not None else [], dtype=str))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            emb = torch.from_numpy(z["embeddings"])
            ids, cats = z["model_ids"].tolist(), z["categories"].tolist()
        if device is not None:
            emb = emb.to(device)
        return cls(emb, ids, cats if len(cats) == len(ids) and len(ids) > 0 else None)
